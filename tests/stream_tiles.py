"""The tile set and the stream of the pipelined multi-handle tests (tests/test_gpu_stream.py, tests/stream_worker.py): what bench.py's timed
stream does -- tiles dealt round-robin over a few region handles, each tile prepared (reset + set_reads + accumulate, nothing waited for) two
ahead of the one being scored -- with the outputs of every tile kept for a comparison with the oracle afterwards."""
import ctypes as C

from uvc_amd import region, synth
from util import INT_GROUPS, presence_violations

# Ten tiles from fixed seeds, 4-12 kb: lengths on both sides of the 4096-position block of the dirty marks (UVC_DIRTY_SHIFT), equal and
# different lengths in a row on one handle, dense and nearly variant-free data next to each other (a stale cell of the tile before shows).
TILES = [
    dict(region_len=12289, depth=120, seed=601, err_rate=0.02, indel_every=150, snv_every=80, clip_frac=0.05),   # SNV- and InDel-dense
    dict(region_len=8192, depth=300, seed=602),                                                  # non-UMI at 300x
    dict(region_len=4097, depth=300, seed=603, umi=True, err_rate=0.03),                         # duplex UMI, noisy bases
    dict(region_len=4095, depth=150, seed=604, indel_every=120),                                 # InDel-dense
    dict(region_len=4097, depth=200, seed=605, umi=True, indel_every=400, err_rate=0.04),        # duplex UMI, InDels, noisy bases
    dict(region_len=12289, depth=300, seed=606),                                                 # non-UMI at 300x
    dict(region_len=8192, depth=100, seed=607, snv_every=60, somatic_every=300),                 # SNV-dense
    dict(region_len=12289, depth=40, seed=608, err_rate=0.0, indel_every=100000, snv_every=100000, somatic_every=0),   # nearly variant-free
    dict(region_len=8192, depth=250, seed=609, umi=True, indel_every=400),                       # duplex UMI
    dict(region_len=8192, depth=40, seed=610, err_rate=0.0, indel_every=100000, snv_every=100000, somatic_every=0),    # nearly variant-free
]
N_HANDLES = 3      # tile k on handle k % 3: each handle is rebound to shorter, longer (within and beyond its size) and equal lengths
AHEAD = 2          # bench.py's default (UVC_BENCH_AHEAD)
KEPT_CAP = 64      # the record buffer of the kept-only stream: most tiles need more (region.py's ENOMEM retry)


def tile_reads(k):
    return synth.generate_region(tid=19, beg=1_000_000 + 100_000 * k, **TILES[k])


def uses_host_reads(k):
    """Every third tile comes from host columns (uvcgpu_region_set_reads), the others from device columns; spread over the handles."""
    return (k + k // 3) % 3 == 2


def library_retried(npos, scored, cap_asked, dev_cap):
    """Whether uvcgpu_region_score's kept-only form needed its second attempt (the device capacity it starts from is the caller's, the handle's
    or (pos_end - pos_beg) / 8 + 4096, whichever is largest) -> (retried, the handle's device capacity afterwards)."""
    cap = max(cap_asked, dev_cap, (npos - 2) // 8 + 4096)
    if scored > cap:
        return True, scored + scored // 8
    return False, cap


def run_stream(lib, reads, cols, release):
    """The stream over all tiles.  release=True: bench.py's finish (score with release_state and kept_only, a small record buffer) -> per tile
    the records plus (scored, capacity asked, whether region.py grew its buffer).  release=False: all-out scoring that keeps the planes, then
    the 14 plane groups of the tile (that fetch syncs only its own handle, after its score: the next two tiles are still in flight) and the
    presence check of those planes (uvcgpu_region_check_presence, called here instead of behind the accumulate).  `cols[k]`: the device columns of tile k (None: host columns)."""
    params = region.default_params(lib)
    Rs = [None] * N_HANDLES
    n = len(reads)
    out = [None] * n

    def prepare(k):
        t, h = reads[k], k % N_HANDLES
        if Rs[h] is None:
            Rs[h] = region.Region(lib, params, t["tid"], t["beg"], t["end"], t["refseq"])
        else:
            Rs[h].reset(t["tid"], t["beg"], t["end"], t["refseq"])
        if cols[k] is None:
            Rs[h].set_reads(t)
        else:
            Rs[h].set_reads_device((cols[k].soa, cols[k]))
        Rs[h].accumulate()

    def finish(k):
        R = Rs[k % N_HANDLES]
        if release:
            grown0 = getattr(R, "_score_cap", 0)
            cap_asked = max(KEPT_CAP, grown0)
            rec = R.score(release_state=True, kept_only=True, capacity=KEPT_CAP)
            sc = C.c_int64()
            lib.dll.uvcgpu_region_last_score_counts(R.h, C.byref(sc), None)
            return dict(records=rec, scored=int(sc.value), cap_asked=cap_asked, enomem=getattr(R, "_score_cap", 0) != grown0)
        rec = R.score(all_out=True)
        planes = {g: R.fetch(g) for g in INT_GROUPS}
        return dict(records=rec, planes=planes, presence=presence_violations(R))

    try:
        for k in range(min(AHEAD, n)):
            prepare(k)
        for k in range(n):
            if k + AHEAD < n:
                prepare(k + AHEAD)
            out[k] = finish(k)
    finally:
        for R in Rs:
            if R is not None:
                R.close()
    return out

