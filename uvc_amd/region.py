"""Host-side mirror of the reference's per-region processing surface (process_batch, main.cpp:458-1193).

    region = Region(lib, params, tid, beg, end, refseq)   # Symbol2CountCoverageSet(tid, beg, end+1), main.cpp:569
    region.set_reads(reads)                               # the alns3 equivalent (UvcReadSoA)
    region.accumulate()                                   # updateByRegion3Aln, main.hpp:3665
    records = region.score(all_out=False)                 # BcfFormat_symbol* call group, main.cpp:648-967
    planes  = region.fetch("SEG32")                       # raw per-position state

`lib` is a `_ffi.Lib`.  The product path binds uvc_amd/csrc/libuvcgpu.so (hand-written HIP for
gfx950); there is NO CPU fallback here -- `gpu_lib()` raises when the extension is missing.
"""
import ctypes as C
import os

import numpy as np

from . import _ffi


class UvcError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("uvc error %d: %s" % (code, msg))
        self.code = code


COVERAGE_MEASURES = _ffi.COVERAGE_MEASURES   # the measures of Region.coverage, in row order: aDP bDP cDP1 cDP12 cDP2 dDP1
CALLABLE_BITS = _ffi.CALLABLE_BITS           # the bits of a mask of Region.callable, in bit order (include/uvc_callable.def)
FAMILY_STATS = _ffi.FAMILY_STATS             # the sections of a row of Region.family_stats, in row order (include/uvc_famstats.def)
FAMILY_CONCORDANCE = _ffi.FAMILY_CONCORDANCE   # the sections of the row of Region.family_concordance, in row order (include/uvc_famconcord.def)
FRAGMENT_PROFILE = _ffi.FRAGMENT_PROFILE     # the sections of the profile row of Region.fragment_profile, in row order (include/uvc_fragprofile.def)
READ_CLASSES = ["R1_fwd", "R1_rev", "R2_fwd", "R2_rev"]   # the read classes of Region.read_profile, in row order (uvcgpu_read_class_name)
ERROR_LEVELS = _ffi.ERROR_LEVELS             # the evidence levels of Region.error_profile, in row order: bDP cDP1 cDP12 cDP2 dDP1
SITE_READ_KINDS = _ffi.SITE_READ_KINDS       # the observation kinds of Region.site_reads, in id order: A C G T N DEL
CLIP_READ = np.dtype([(n, np.int32) for n, _ in _ffi.UvcClipRead._fields_])   # UvcClipRead: site read soft_len hard_len
CLIP_MATE = np.dtype([(n, np.int32) for n, _ in _ffi.UvcClipMate._fields_])   # UvcClipMate: site read cluster klass
SITE_READ = np.dtype([(n, np.int32) for n, _ in _ffi.UvcSiteRead._fields_])   # UvcSiteRead: site read q obs ins_q ins_len del_len reserved
CALLABLE_RUN = np.dtype([("range", np.int32), ("pos_beg", np.int32), ("pos_end", np.int32), ("mask", np.int32)])   # UvcCallableRun

_gpu_lib = None


def gpu_lib():
    """Loads libuvcgpu.so and initialises device 0.  Fails loudly when the extension or the GPU is missing."""
    global _gpu_lib
    if _gpu_lib is None:
        import os
        path = _ffi.gpu_library_path()
        if not os.path.exists(path):
            raise ImportError("HIP extension %s is not built: run `python -c 'import __graft_entry__ as g; g.build()'`" % path)
        lib = _ffi.Lib(path, "uvcgpu_")
        lib.dll.uvcgpu_init.restype, lib.dll.uvcgpu_init.argtypes = C.c_int, [C.c_int]
        _gpu_lib = lib
    return _gpu_lib


def default_params(lib, platform=1, central_readlen=150, max_mapq=60):
    """Reference defaults + the platform deltas of CommandLineArgs::selfUpdateByPlatform (CmdLineArgs.cpp:113-134)."""
    p = _ffi.UvcParams()
    lib.call("params_default", C.byref(p))
    apply_platform(p, platform, central_readlen, max_mapq)
    return p


def apply_platform(p, platform, central_readlen, max_mapq):
    # CmdLineArgs.cpp:13-15, 113-134
    p.inferred_sequencing_platform = platform
    if p.central_readlen == 0:
        p.central_readlen = central_readlen
    p.inferred_maxMQ = max(p.inferred_maxMQ, max_mapq)
    if platform == 2:    # IonTorrent
        p.bq_phred_added_misma += 8
        for name, dec in (("fam_thres_highBQ_snv", 30), ("fam_thres_highBQ_indel", 30), ("bias_thres_PFBQ1", 30), ("bias_thres_PFBQ2", 30), ("bias_thres_highBQ", 13)):
            v = getattr(p, name)
            setattr(p, name, v - min(v, dec))
    elif platform == 1:  # Illumina
        p.syserr_minABQ_pcr_snv += 200
        p.syserr_minABQ_pcr_indel += 100
        p.syserr_minABQ_cap_snv += 200
        p.syserr_minABQ_cap_indel += 100


def _param_fn(name, restype, argtypes):
    f = getattr(gpu_lib().dll, "uvcgpu_" + name)
    f.restype, f.argtypes = restype, argtypes
    return f


def param_table():
    """Every row of include/uvc_params.def, then of include/uvc_group_params.def (uvcgpu_param_info): list of dicts name, kind ("int" /
    "double"), owner ("params" / "group"), default, settable (False for the derived rows inferred_*, tumor_vcf_*)."""
    info = _param_fn("param_info", C.c_int, [C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int32)])
    rows = []
    for i in range(_param_fn("param_count", C.c_int32, [])()):
        name, kind, owner, dflt, settable = C.c_char_p(), C.c_int32(), C.c_int32(), C.c_double(), C.c_int32()
        if info(i, C.byref(name), C.byref(kind), C.byref(owner), C.byref(dflt), C.byref(settable)) != 0:
            raise UvcError(_ffi.ENUMS["UVCGPU_EINVAL"], gpu_lib().last_error())
        rows.append(dict(name=name.value.decode(), kind=("int" if kind.value == _ffi.ENUMS["UVC_PARAM_INT"] else "double"),
                         owner=("group" if owner.value == _ffi.ENUMS["UVC_PARAM_OF_GROUP"] else "params"),
                         default=(int(dflt.value) if kind.value == _ffi.ENUMS["UVC_PARAM_INT"] else dflt.value), settable=bool(settable.value)))
    return rows


def set_param(params, group_params, name, value):
    """uvcgpu_param_set: the row `name` (field or option form) of `params` (a _ffi.UvcParams) or `group_params` (a group.UvcGroupParams; either
    may be None when the row is not its) from `value` (a number, a bool or its text), parsed as the command line parses it.  Raises UvcError."""
    if isinstance(value, bool):
        value = int(value)
    text = repr(float(value)) if isinstance(value, float) else str(value)
    f = _param_fn("param_set", C.c_int, [C.c_void_p, C.c_void_p, C.c_char_p, C.c_char_p])
    rc = f(C.addressof(params) if params is not None else None, C.addressof(group_params) if group_params is not None else None, name.encode(), text.encode())
    if rc != 0:
        raise UvcError(rc, gpu_lib().last_error())


def apply_platform_ex(params, sequencing_platform, inferred, central_readlen, max_mapq):
    """uvcgpu_params_apply_platform_ex: the platform step of a requested --sequencing-platform (0 AUTO, 1 ILLUMINA, 2 IONTORRENT, 3 OTHER)."""
    f = _param_fn("params_apply_platform_ex", C.c_int, [C.POINTER(_ffi.UvcParams), C.c_int32, C.c_int32, C.c_int32, C.c_int32])
    rc = f(C.byref(params), sequencing_platform, inferred, central_readlen, max_mapq)
    if rc != 0:
        raise UvcError(rc, gpu_lib().last_error())


_READ_FIELDS = [("pos", np.int32), ("mpos", np.int32), ("isize", np.int32), ("flag", np.uint16), ("mapq", np.uint8), ("nm", np.int32),
                ("l_qseq", np.int32), ("seq_off", np.int64), ("cigar_off", np.int64), ("n_cigar", np.int32),
                ("frag_id", np.int32), ("fam_id", np.int32), ("fam_strand", np.uint8)]


_NT16 = np.array([1, 2, 4, 8, 15], dtype=np.uint8)   # A C G T N as BAM's 4-bit codes (seq_nt16_str "=ACMGRSVTWYHKDBN")


def compact_form(reads):
    """The same reads in the compact input form of UvcReadSoA: `bases4` = the bases as a BAM record holds them (two 4-bit codes per byte, high
    nibble first, every read on a byte boundary, reads back to back) instead of one byte per base, and no seq_off / cigar_off columns (the
    library derives them on the device).  Needs the reads back to back in read order, which is how every packer here lays them out."""
    n = int(reads["n_reads"])
    lq = np.asarray(reads["l_qseq"], dtype=np.int64)
    nc = np.asarray(reads["n_cigar"], dtype=np.int64)
    so = np.concatenate(([0], np.cumsum(lq)))[:n]
    co = np.concatenate(([0], np.cumsum(nc)))[:n]
    if not (np.array_equal(so, np.asarray(reads["seq_off"])) and np.array_equal(co, np.asarray(reads["cigar_off"]))):
        raise ValueError("compact_form needs reads that lie back to back in read order")
    codes = _NT16[np.minimum(np.asarray(reads["bases"], dtype=np.uint8), 4)]
    nb = (lq + 1) // 2
    bo = np.concatenate(([0], np.cumsum(nb)))
    if n and not (lq % 2).any():                                     # every read starts on an even base index: two neighbours per byte
        out4 = (codes[0::2] << 4) | codes[1::2]
    else:
        out4 = np.zeros(int(bo[-1]), dtype=np.uint8)
        if n:
            k = np.arange(int(lq.sum())) - np.repeat(so, lq)            # index of every base inside its read
            byte = np.repeat(bo[:n], lq) + k // 2
            hi = (k % 2 == 0)
            out4[byte[hi]] = codes[hi] << 4                              # each byte has one high and at most one low nibble
            out4[byte[~hi]] |= codes[~hi]
    c = {k_: v for k_, v in reads.items() if k_ not in ("bases", "seq_off", "cigar_off")}
    c["bases4"] = out4
    return c


def _fill_soa(reads, put):
    """UvcReadSoA from a dict of columns; `put(array, dtype) -> address` places a column (host or device).  Columns a compact dict leaves
    out (seq_off, cigar_off, bases) stay NULL."""
    soa = _ffi.UvcReadSoA()
    soa.struct_size = C.sizeof(_ffi.UvcReadSoA)
    soa.n_reads = int(reads["n_reads"])
    for name, dt in _READ_FIELDS:
        if name in ("seq_off", "cigar_off") and reads.get(name) is None:
            continue
        a = np.ascontiguousarray(reads[name], dtype=dt)
        assert a.shape == (soa.n_reads,), name
        setattr(soa, name, put(a, dt))
    soa.n_bases = int(np.asarray(reads["quals"]).size)
    soa.n_cigar_ops = int(np.asarray(reads["cigars"]).size)
    soa.quals = put(reads["quals"], np.uint8)
    soa.cigars = put(reads["cigars"], np.uint32)
    if reads.get("bases") is not None:
        soa.bases = put(reads["bases"], np.uint8)
    else:
        soa.bases4 = put(reads["bases4"], np.uint8)
        soa.n_bases4_bytes = int(np.asarray(reads["bases4"]).size)
    soa.n_fams = int(reads["n_fams"])
    soa.fam_dflag = put(reads["fam_dflag"], np.uint8)
    return soa


def pack_reads(reads):
    """dict of numpy arrays -> (UvcReadSoA, keepalive list)."""
    keep = []

    def put(a, dt):
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        return a.ctypes.data
    return _fill_soa(reads, put), keep


def device_reads(reads, device):
    """The UvcReadSoA columns of `reads` as torch tensors on `device` (torch is only the owner of the HBM here) -> (UvcReadSoA of device
    pointers, keepalive) for Region.set_reads_device: what a caller has whose decoder writes straight to the GPU.
    torch ships its own copy of the HIP runtime: initialise torch.cuda BEFORE libuvcgpu.so touches the device (bench.py does), the other
    order leaves torch without a GPU.  Without torch, allocate through the runtime the library links (tests/test_gpu_device_reads.py)."""
    import torch
    keep = []

    def put(a, dt):
        a = np.ascontiguousarray(a, dtype=dt)
        # torch has no uint16 / uint32 tensors everywhere: ship the bytes
        t = torch.from_numpy(a.view(np.uint8).reshape(-1)).to(device)
        keep.append(t)
        return t.data_ptr() if t.numel() else 0
    soa = _fill_soa(reads, put)
    torch.cuda.synchronize(device)
    return soa, keep


def vcf_format_keys(lib, tier2=False):
    fn = getattr(lib.dll, "uvcgpu_vcf_format_keys")
    fn.restype, fn.argtypes = C.c_char_p, [C.c_int32]
    return fn(int(tier2)).decode()


def vcf_header(lib, params, sample, contigs, tumor_sample=None):
    """##-lines and the #CHROM line (uvcgpu_vcf_header); contigs = [(name, length), ...]; tumor_sample: the second sample column of a
    normal-sample VCF that carries the tumor's FORMAT over (is_tumor_format_retrieved)."""
    fn = getattr(lib.dll, "uvcgpu_vcf_header")
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(_ffi.UvcParams), C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    names = (C.c_char_p * max(1, len(contigs)))(*[c[0].encode() for c in contigs])
    lens = (C.c_int64 * max(1, len(contigs)))(*[int(c[1]) for c in contigs])
    ln = C.c_int64(0)
    ts = tumor_sample.encode() if tumor_sample else None
    fn(C.byref(params), sample.encode(), ts, names, lens, len(contigs), None, 0, C.byref(ln))
    dst = C.create_string_buffer(max(1, ln.value))
    rc = fn(C.byref(params), sample.encode(), ts, names, lens, len(contigs), dst, ln.value, C.byref(ln))
    if rc:
        raise UvcError(rc, lib.last_error())
    return dst.raw[:ln.value].decode()


def _coverage_ranges(ranges):
    """(pos_beg, pos_end) pairs as the UvcCoverageRange array of the plane readers (at least one element: an empty list still has an
    address), and the pairs as ints."""
    rows = [(int(q[0]), int(q[1])) for q in ranges]
    return (_ffi.UvcCoverageRange * max(len(rows), 1))(*[_ffi.UvcCoverageRange(*q) for q in rows]), rows


class Region:
    def __init__(self, lib, params, tid, beg, end, refseq):
        self.lib, self.tid, self.beg, self.end = lib, tid, beg, end
        self.npos = end - beg + 1
        self.h = C.c_void_p()
        self._params = params
        ref = refseq.encode() if isinstance(refseq, str) else bytes(refseq)
        if len(ref) != end - beg:
            raise ValueError("refseq must cover [beg, end)")
        self._check(lib.call("create", C.byref(self.h), C.byref(params), tid, beg, end, ref))

    def _check(self, rc):
        if rc != 0:
            raise UvcError(rc, self.lib.last_error())

    def reset(self, tid, beg, end, refseq):
        """Re-binds the handle to another region (uvcgpu_region_reset): streams and, if the region is not longer, device buffers are kept.
        Libraries without that entry point (the test oracle) get a fresh handle instead."""
        ref = refseq.encode() if isinstance(refseq, str) else bytes(refseq)
        if len(ref) != end - beg:
            raise ValueError("refseq must cover [beg, end)")
        fn = getattr(self.lib.dll, self.lib.prefix + "region_reset", None)
        if fn is None:
            self.close()
            self._check(self.lib.call("create", C.byref(self.h), C.byref(self._params), tid, beg, end, ref))
        else:
            fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_char_p]
            self._check(fn(self.h, tid, beg, end, ref))
        self.tid, self.beg, self.end, self.npos = tid, beg, end, end - beg + 1   # (the records buffer stays: score() replaces it when the capacity asked for changes)

    def set_reads(self, reads):
        soa, keep = pack_reads(reads)
        self._check(self.lib.call("set_reads", self.h, C.byref(soa)))

    def set_reads_device(self, dev):
        """uvcgpu_region_set_reads_device: `dev` = (UvcReadSoA of device pointers, keepalive) as `device_reads` makes it.  The arrays must
        outlive the reads of the handle."""
        soa, keep = dev
        fn = getattr(self.lib.dll, self.lib.prefix + "region_set_reads_device")
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(_ffi.UvcReadSoA)]
        self._dev_reads = keep
        self._check(fn(self.h, C.byref(soa)))

    def accumulate(self):
        self._check(self.lib.call("accumulate", self.h))
        if os.environ.get("UVCGPU_CHECK_PRESENCE") and hasattr(self.lib.dll, self.lib.prefix + "region_check_presence"):
            # the test suite's switch: the planes of every accumulate against the presence statement the scoring gather relies on
            n = C.c_int64(-1)
            fn = getattr(self.lib.dll, self.lib.prefix + "region_check_presence")
            fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]
            self._check(fn(self.h, C.byref(n)))
            if n.value != 0:
                raise AssertionError("uvcgpu_region_check_presence: %d (position, symbol) cells contradict the presence statement" % n.value)

    def correct_bq(self):
        """apply_bq_err_correction3 (grouping.cpp:459-543) on the library's copy of the base qualities."""
        fn = getattr(self.lib.dll, self.lib.prefix + "region_correct_bq")
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p]
        self._check(fn(self.h))

    def debug_mis_queue(self):
        """For tests: the mismatch queue of the last accumulate (uvcgpu_region_debug_mis_queue) -> (rows [n][rank, epos, symval] in the
        device's order, the device's count n, the count set_reads made)."""
        fn = getattr(self.lib.dll, self.lib.prefix + "region_debug_mis_queue")
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        n, total = C.c_int64(-1), C.c_int64(-1)
        self._check(fn(self.h, None, 0, C.byref(n), C.byref(total)))
        rows = np.empty((max(int(n.value), 0), 3), dtype=np.int32)
        self._check(fn(self.h, rows.ctypes.data, rows.shape[0], C.byref(n), C.byref(total)))
        return rows[:max(min(int(n.value), rows.shape[0]), 0)], int(n.value), int(total.value)

    def read_quals(self, n_bases):
        fn = getattr(self.lib.dll, self.lib.prefix + "region_read_quals")
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]
        out = np.empty(n_bases, dtype=np.uint8)
        self._check(fn(self.h, out.ctypes.data, n_bases))
        return out

    def fetch(self, group):
        gid, dt, shape = _ffi.FIELD_GROUPS[group]
        nbytes = self.lib.call("field_bytes", self.h, gid)
        if nbytes < 0:
            raise UvcError(-5, "field group %s not available" % group)
        out = np.empty(shape + (self.npos,), dtype=dt)
        assert out.nbytes == nbytes, (group, out.nbytes, nbytes)
        self._check(self.lib.call("fetch", self.h, gid, out.ctypes.data, out.nbytes))
        return out

    def indel_alleles(self):
        """The per-strand InDel allele rows fill_by_indel_info reads (instcode.hpp): list of dicts with the inserted sequence as text
        (insertions) or None (deletions: the deleted bases are refseq[refpos - beg : + len])."""
        fn = getattr(self.lib.dll, self.lib.prefix + "region_indel_alleles")
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        n, nb = C.c_int64(0), C.c_int64(0)
        rc = fn(self.h, None, 0, C.byref(n), None, 0, C.byref(nb))
        if rc not in (0, -6):
            self._check(rc)
        rows = (_ffi.UvcGapRow * max(1, n.value))()
        seq = np.zeros(max(1, nb.value), dtype=np.uint8)
        self._check(fn(self.h, rows, n.value, C.byref(n), seq.ctypes.data, nb.value, C.byref(nb)))
        out = []
        for i in range(n.value):
            r = rows[i]
            text = "".join("ACGTN"[b] for b in seq[r.seq_off:r.seq_off + r.len]) if r.seq_off >= 0 else None
            out.append(dict(refpos=r.refpos, symbol=r.symbol, strand=r.strand, len=r.len, seq=text, bAD1=r.bAD1, cAD1=r.cAD1, c2AD=r.c2AD, c2dAD=r.c2dAD))
        return out

    @staticmethod
    def make_request(all_out=False, pos_beg=-1, pos_end=-1, is_amplicon=False, indel_alleles=None, tumor_keys=None, release_state=False, base_at_pos_beg=False, region_beg=0,
                     tumor_sample_columns=None, tumor_ref_alt=None, kept_only=False, force_sites=None):
        """UvcScoreRequest + the ctypes arrays it points into (keep both alive for the call).  `force_sites`: zerobased_pos values (= the VCF
        POS of the records they select) whose (position, symbol type) groups are scored as with all_out; sorted and de-duplicated here."""
        req = _ffi.UvcScoreRequest()
        req.pos_beg, req.pos_end, req.all_out, req.is_amplicon = pos_beg, pos_end, int(all_out), int(is_amplicon)
        req.release_state = int(release_state)   # the planes may be zeroed for the next accumulate as soon as the scoring kernels are done
        req.base_at_pos_beg, req.region_beg = int(base_at_pos_beg), int(region_beg)
        req.kept_only = int(kept_only)           # only the (position, symbol type) groups the record writer reads
        arr = None
        if indel_alleles:
            arr = (_ffi.UvcIndelAllele * len(indel_alleles))(*[_ffi.UvcIndelAllele(*a) for a in indel_alleles])
            req.n_indel_alleles, req.indel_alleles = len(indel_alleles), C.cast(arr, C.c_void_p)
        tk = None
        if tumor_keys is not None and len(tumor_keys):   # T/N: UvcTumorKey field tuples (or a ready ctypes array), sorted by (refpos, symbol)
            tk = tumor_keys if isinstance(tumor_keys, C.Array) else (_ffi.UvcTumorKey * len(tumor_keys))(*[_ffi.UvcTumorKey(*t) for t in tumor_keys])
            req.n_tumor_keys, req.tumor_keys = len(tk), C.cast(tk, C.c_void_p)
        cols = None
        if tk is not None and tumor_sample_columns:   # is_tumor_format_retrieved: the tumor's sample column of every key, appended by the record writer
            assert len(tumor_sample_columns) == len(tk)
            cols = (C.c_char_p * len(tk))(*[c.encode() if isinstance(c, str) else c for c in tumor_sample_columns])
            req.tumor_sample_columns = C.cast(cols, C.c_void_p)
        ras = None
        if tk is not None and tumor_ref_alt:          # "REF\tALT" of every key: the InDel strings of rescued InDel records (record writer)
            assert len(tumor_ref_alt) == len(tk)
            ras = (C.c_char_p * len(tk))(*[c.encode() if isinstance(c, str) else c for c in tumor_ref_alt])
            req.tumor_ref_alt = C.cast(ras, C.c_void_p)
        fs = None
        if force_sites is not None and len(force_sites):
            fs = np.ascontiguousarray(np.unique(np.asarray(force_sites, dtype=np.int64)).astype(np.int32))
            req.n_force_sites, req.force_sites = len(fs), fs.ctypes.data
        return req, (arr, tk, cols, ras, fs)

    def hap_links(self):
        """hap_bq / hap_fq / hap_f2q of updateByRegion3Aln (uvcgpu_region_hap_links): three lists of (mutations, (fwd, rev), (other fwd, other rev))
        with mutations = ((refpos, symbol), ...)."""
        fn = getattr(self.lib.dll, self.lib.prefix + "region_hap_links")
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        n, m = C.c_int64(0), C.c_int64(0)
        rc = fn(self.h, None, 0, C.byref(n), None, 0, C.byref(m))
        if rc not in (0, -6):
            self._check(rc)
        links = (_ffi.UvcHapLink * max(1, n.value))()
        muts = np.zeros(max(1, m.value), dtype=np.int32)
        self._check(fn(self.h, links, n.value, C.byref(n), muts.ctypes.data, m.value, C.byref(m)))
        out = [[], [], []]
        for i in range(n.value):
            l = links[i]
            pairs = tuple((int(muts[l.mut_off + 2 * k]), int(muts[l.mut_off + 2 * k + 1])) for k in range(l.n_muts))
            out[l.which].append((pairs, (l.fr_cnt[0], l.fr_cnt[1]), (l.other_cnt[0], l.other_cnt[1])))
        return out

    def score(self, all_out=False, pos_beg=-1, pos_end=-1, is_amplicon=False, indel_alleles=None, capacity=None, copy=True, tumor_keys=None, release_state=False, base_at_pos_beg=False, region_beg=0,
              kept_only=False, force_sites=None):
        req, _keep = self.make_request(all_out, pos_beg, pos_end, is_amplicon, indel_alleles, tumor_keys, release_state, base_at_pos_beg, region_beg, kept_only=kept_only,
                                       force_sites=force_sites)
        if capacity is None:
            npos = (pos_end - pos_beg) if pos_beg >= 0 else self.npos
            capacity = 14 * (npos + 1) if all_out else max(4096, 4 * (npos + 1)) + 16 * int(req.n_force_sites)
        capacity = max(capacity, getattr(self, "_score_cap", 0))   # a handle that needed a larger buffer once asks for it at once the next time
        while True:
            buf = getattr(self, "_score_buf", None)   # reused across calls: the library fills n_records columns of every row
            if buf is None or buf.shape[1] != capacity:
                self._free_score_buf()
                buf = self._score_buf = self._alloc_score_buf(capacity)
            out = _ffi.UvcScoreOut(capacity, 0, buf.ctypes.data)
            rc = self.lib.call("score", self.h, C.byref(req), C.byref(out))
            if rc == -6 and out.n_records > capacity:
                capacity = self._score_cap = int(out.n_records) + int(out.n_records) // 8
                continue
            self._check(rc)
            # copy=False returns views into the handle's reusable buffer (valid until the next score() call)
            return {name: (buf[i, :out.n_records].copy() if copy else buf[i, :out.n_records]) for i, name in enumerate(_ffi.SCORE_FIELDS)}

    @staticmethod
    def make_ranges(ranges):
        """UvcScoreRange array from (pos_beg, pos_end[, base_at_pos_beg[, region_beg]]) tuples."""
        rows = [tuple(int(v) for v in q) + (0,) * (4 - len(q)) for q in ranges]
        return (_ffi.UvcScoreRange * max(len(rows), 1))(*[_ffi.UvcScoreRange(*q) for q in rows]), len(rows)

    def _ranges_fn(self, name, restype, argtypes):
        """The ranges entry points exist in the HIP library only: bound on first use."""
        fn = getattr(self.lib.dll, self.lib.prefix + name, None)
        if fn is None:
            raise UvcError(_ffi.ENUMS["UVCGPU_EUNSUPPORTED"], "%s has no %s%s" % (self.lib.path, self.lib.prefix, name))
        fn.restype, fn.argtypes = restype, argtypes
        return fn

    def score_ranges(self, ranges, all_out=False, is_amplicon=False, indel_alleles=None, capacity=None, copy=True, tumor_keys=None, release_state=False, kept_only=False, force_sites=None):
        """uvcgpu_region_score_ranges: the records of score() called once per range -- (pos_beg, pos_end[, base_at_pos_beg[, region_beg]]),
        sorted and disjoint -- on this accumulated handle, concatenated in range order, from one gate, one set of launches and one D2H."""
        fn = self._ranges_fn("region_score_ranges", C.c_int, [C.c_void_p, C.POINTER(_ffi.UvcScoreRequest), C.c_void_p, C.c_int64, C.POINTER(_ffi.UvcScoreOut)])
        req, _keep = self.make_request(all_out, -1, -1, is_amplicon, indel_alleles, tumor_keys, release_state, kept_only=kept_only, force_sites=force_sites)
        arr, n = self.make_ranges(ranges)
        if capacity is None:
            npos = sum(max(0, int(q[1]) - int(q[0])) for q in ranges)
            capacity = 14 * (npos + 1) if all_out else max(4096, 4 * (npos + 1)) + 16 * int(req.n_force_sites)
        capacity = max(capacity, getattr(self, "_score_cap", 0))
        while True:
            buf = getattr(self, "_score_buf", None)
            if buf is None or buf.shape[1] != capacity:
                self._free_score_buf()
                buf = self._score_buf = self._alloc_score_buf(capacity)
            out = _ffi.UvcScoreOut(capacity, 0, buf.ctypes.data)
            rc = fn(self.h, C.byref(req), arr, n, C.byref(out))
            if rc == -6 and out.n_records > capacity:
                capacity = self._score_cap = int(out.n_records) + int(out.n_records) // 8
                continue
            self._check(rc)
            return {name: (buf[i, :out.n_records].copy() if copy else buf[i, :out.n_records]) for i, name in enumerate(_ffi.SCORE_FIELDS)}

    def score_stream(self, chunk_records, ranges=None, copy=True, all_out=False, pos_beg=-1, pos_end=-1, is_amplicon=False, indel_alleles=None, tumor_keys=None, release_state=False,
                     base_at_pos_beg=False, region_beg=0, kept_only=False, force_sites=None):
        """The records of score(...) -- or, with `ranges`, of score_ranges(ranges, ...) -- in bounded memory (uvcgpu_region_score_stream_begin /
        uvcgpu_score_stream_next / uvcgpu_score_stream_end): a generator of (records, covered_ranges), one pair per chunk of at most
        `chunk_records` records.  A chunk is a run of whole positions; its records are those of score_ranges(covered_ranges) and
        vcf_records_ranges(contig, records, covered_ranges) is its text; the chunks' records and texts concatenate to the one call's (germ_ref /
        germ_alt1 / germ_alt2 count from the chunk's first record).  copy=False yields views into the stream's page-locked buffer, valid until
        the generator is advanced.  Closing the generator early ends the stream."""
        begin = self._ranges_fn("region_score_stream_begin", C.c_int, [C.c_void_p, C.POINTER(_ffi.UvcScoreRequest), C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.c_void_p)])
        nxt = self._ranges_fn("score_stream_next", C.c_int, [C.c_void_p, C.POINTER(_ffi.UvcScoreOut), C.c_void_p, C.POINTER(C.c_int64)])
        end = self._ranges_fn("score_stream_end", C.c_int, [C.c_void_p])
        if ranges is not None:
            pos_beg, pos_end, base_at_pos_beg, region_beg = -1, -1, False, 0
        req, _keep = self.make_request(all_out, pos_beg, pos_end, is_amplicon, indel_alleles, tumor_keys, release_state, base_at_pos_beg, region_beg, kept_only=kept_only, force_sites=force_sites)
        arr, n = self.make_ranges(ranges) if ranges is not None else (None, 0)
        h = C.c_void_p()
        self._check(begin(self.h, C.byref(req), arr, n, int(chunk_records), C.byref(h)))
        try:
            covered = (_ffi.UvcScoreRange * max(n, 1))()
            while True:
                out, nc = _ffi.UvcScoreOut(), C.c_int64(0)
                rc = nxt(h, C.byref(out), covered, C.byref(nc))
                if rc == _ffi.ENUMS["UVCGPU_STREAM_END"]:
                    break
                self._check(rc)
                buf = np.ctypeslib.as_array((C.c_int32 * (_ffi.NUM_SCORE_FIELDS * out.capacity)).from_address(out.fields)).reshape(_ffi.NUM_SCORE_FIELDS, out.capacity)
                rec = {name: (buf[i, :out.n_records].copy() if copy else buf[i, :out.n_records]) for i, name in enumerate(_ffi.SCORE_FIELDS)}
                yield rec, [(q.pos_beg, q.pos_end, q.base_at_pos_beg, q.region_beg) for q in covered[:nc.value]]
        finally:
            end(h)

    def coverage(self, ranges, thresholds=()):
        """uvcgpu_region_coverage: depth statistics of `ranges` -- (pos_beg, pos_end) pairs, zero-based, half open, sorted and disjoint, inside
        the region -- reduced on the device from the accumulated planes.  int64 [n_ranges, UVC_NCOV, 3 + n_thresholds]: per measure of
        COVERAGE_MEASURES the sum, the minimum and the maximum of its per-position depth over the range, then the number of positions at or
        above each of `thresholds` (at most 8, ascending).  After accumulate() and before anything that releases the planes."""
        fn = self._ranges_fn("region_coverage", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p])
        arr, rows = _coverage_ranges(ranges)
        thr = np.ascontiguousarray(thresholds, dtype=np.int32).reshape(-1)
        ncov, row = _ffi.ENUMS["UVC_NCOV"], _ffi.ENUMS["UVC_COV_ROW"]
        out = np.zeros((max(len(rows), 1), ncov, row), dtype=np.int64)
        self._check(fn(self.h, arr, len(rows), thr.ctypes.data if len(thr) else None, len(thr), out.ctypes.data))
        return out[:len(rows), :, :_ffi.ENUMS["UVC_COV_GE"] + len(thr)].copy()

    def error_profile(self, ranges, min_depth=20, max_alt_permille=50):
        """uvcgpu_region_error_profile: the background error profile of `ranges` (as Region.coverage takes them), reduced on the device from the
        accumulated planes.  int64 [UVC_NERRLEVEL, UVC_ERR_ROW]: per level of ERROR_LEVELS 256 BASE bins [ctx][A C G T], 448 LINK bins
        [ctx][M D3P D2 D1 I3P I2 I1] and 8 counters (UvcErrCounter), ctx = 16 l + 4 m + r of the reference symbols around the position; a
        position enters a level's bins where the level's depth is >= min_depth and its largest non-reference count is at most max_alt_permille
        thousandths of it (uvcgpu.h has the rules).  After accumulate() and before anything that releases the planes."""
        fn = self._ranges_fn("region_error_profile", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p])
        arr, rows = _coverage_ranges(ranges)
        req = _ffi.UvcErrorProfileRequest(int(min_depth), int(max_alt_permille))
        out = np.zeros((_ffi.ENUMS["UVC_NERRLEVEL"], _ffi.ENUMS["UVC_ERR_ROW"]), dtype=np.int64)
        self._check(fn(self.h, arr, len(rows), C.byref(req), out.ctypes.data))
        return out

    def family_stats(self, ranges):
        """uvcgpu_region_family_stats: family-size statistics of `ranges` -- rows of (pos_beg, pos_end[, prev_end[, flags]]), zero-based, half
        open, sorted and disjoint, inside the region; prev_end (default: pos_beg) <= pos_beg, not decreasing and not below the end of the range
        before; flags bit 0 = the range continues the target of the range before -- reduced on the device from the family units of the
        region's reads.  int64 [n_ranges, UVC_FAMSTAT_ROW]: the TARGET block (families, fragments, alignments, families on both strands, of the
        families that overlap the range) and the FIRST block (the same, three flag counters, a reserved word, size[64], strands[17][17], of
        the families that overlap it and begin at or behind prev_end); FAMILY_STATS names the sections, uvcgpu.h has the rules.  After
        set_reads() / set_reads_device(); accumulate and scores neither are needed nor get in the way."""
        fn = self._ranges_fn("region_family_stats", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p])
        rows = [(int(q[0]), int(q[1]), int(q[2]) if len(q) > 2 else int(q[0]), int(q[3]) if len(q) > 3 else 0) for q in ranges]
        arr = (_ffi.UvcFamilyRange * max(len(rows), 1))(*[_ffi.UvcFamilyRange(*q) for q in rows])
        out = np.zeros((len(rows), _ffi.ENUMS["UVC_FAMSTAT_ROW"]), dtype=np.int64)
        self._check(fn(self.h, arr, len(rows), out.ctypes.data))
        return out

    def family_concordance(self, ranges):
        """uvcgpu_region_family_concordance: what the family consensus out-voted and where the strands of a duplex family disagree, over
        `ranges` (as Region.coverage takes them).  int64 [UVC_FAMCONC_ROW], every word a sum over the (unit, position) pairs of the ranges:
        base[refclass][bin][consensus][vote] and link[bin][consensus][vote] (the votes of a unit's fragments by the unit's consensus symbol
        and the bin 1, 2, 3, 4, 5-7, 8-15, 16-31, 32+ of its vote total), base_pos / link_pos (positions, unanimous positions),
        dup_base[ref][strand-0 vote][strand-1 vote] and dup_link (the two votes of the duplex pass, the last index: none) and 16 counters;
        FAMILY_CONCORDANCE names the sections, uvcgpu.h has the rules.  The votes are evaluated again on the device: after accumulate() of
        the current reads, whatever was scored since."""
        fn = self._ranges_fn("region_family_concordance", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p])
        arr, rows = _coverage_ranges(ranges)
        out = np.zeros(_ffi.ENUMS["UVC_FAMCONC_ROW"], dtype=np.int64)
        self._check(fn(self.h, arr, len(rows), out.ctypes.data))
        return out

    def fragment_profile(self, ranges, min_mapq=0, short=(100, 150), long=(151, 220)):
        """uvcgpu_region_fragment_profile: template lengths and reference end motifs of the fragments and families of `ranges` (rows as
        family_stats takes them), reduced on the device from the alignment columns, the fragments and the family units of the region's
        reads.  -> (rows, profile): rows int64 [n_ranges, UVC_FRAGPROF_TARGET_ROW] (pairs, others, singles, len_sum, short, long, families,
        a reserved 0, of the objects that overlap the range) and profile int64 [UVC_FRAGPROF_ROW] (the same words, families_both_strands,
        ends, ends_off_region, ends_no_ref, LEN[1024], FAMLEN[1024], MOTIF[256], of the objects that overlap a range and begin at or behind
        its prev_end: once per call); FRAGMENT_PROFILE names the sections, uvcgpu.h has the rules.  An alignment counts with
        mapq >= min_mapq and none of the flags 0x904; `short` / `long` are inclusive bounds of the template length.  Legal where
        family_stats() is."""
        fn = self._ranges_fn("region_fragment_profile", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p])
        rows = [(int(q[0]), int(q[1]), int(q[2]) if len(q) > 2 else int(q[0]), int(q[3]) if len(q) > 3 else 0) for q in ranges]
        arr = (_ffi.UvcFamilyRange * max(len(rows), 1))(*[_ffi.UvcFamilyRange(*q) for q in rows])
        req = _ffi.UvcFragmentProfileRequest(int(min_mapq), int(short[0]), int(short[1]), int(long[0]), int(long[1]))
        out = np.zeros((len(rows), _ffi.ENUMS["UVC_FRAGPROF_TARGET_ROW"]), dtype=np.int64)
        prof = np.zeros(_ffi.ENUMS["UVC_FRAGPROF_ROW"], dtype=np.int64)
        self._check(fn(self.h, arr, len(rows), C.byref(req), out.ctypes.data, prof.ctypes.data))
        return out, prof

    def read_profile(self, ranges, min_mapq=0, min_depth=20, max_alt_permille=50):
        """uvcgpu_region_read_profile: the base-quality, cycle and substitution profile of the region's reads over `ranges` (as Region.coverage
        takes them), reduced on the device from the read bases.  int64 [UVC_READPROF_ROW]: Q[4][64][2] (class of READ_CLASSES, quality bin,
        match / mismatch), CYC[4][256][5] (class, cycle bin, match / mismatch / ins / del / clip), SUB[4][4][4] (class, reference base, read
        base) and 16 counters (_ffi.READPROF_SECTIONS names the sections, uvcgpu.h has the rules).  An alignment counts with
        mapq >= min_mapq; a base enters the bins at a position whose depth of counted A/C/G/T bases is >= min_depth and whose mismatches are
        at most max_alt_permille thousandths of it.  After set_reads() / set_reads_device(); accumulate and scores neither are needed nor get
        in the way; after correct_bq() the qualities are the corrected ones."""
        fn = self._ranges_fn("region_read_profile", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p])
        arr, rows = _coverage_ranges(ranges)
        req = _ffi.UvcReadProfileRequest(int(min_mapq), int(min_depth), int(max_alt_permille))
        out = np.zeros(_ffi.ENUMS["UVC_READPROF_ROW"], dtype=np.int64)
        self._check(fn(self.h, arr, len(rows), C.byref(req), out.ctypes.data))
        return out

    def callable(self, ranges, min_depth=None, max_aDP=0):
        """uvcgpu_region_callable: the runs of equal callability masks of `ranges` -- (pos_beg, pos_end) pairs as for coverage().  min_depth:
        measure name of COVERAGE_MEASURES -> smallest depth (0 or absent: not tested); max_aDP: largest raw depth (0: not tested).  A
        structured array (range, pos_beg, pos_end, mask; int32), sorted by (range, pos_beg), the runs of a range tiling it; bit k of mask is
        CALLABLE_BITS[k], mask 0 = callable.  Classified and compacted on the device; asks for the size first, then for the runs."""
        fn = self._ranges_fn("region_callable", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p])
        arr, rows = _coverage_ranges(ranges)
        req = _ffi.UvcCallableRequest()
        for name, v in (min_depth or {}).items():
            req.min_depth[COVERAGE_MEASURES.index(name)] = int(v)
        req.max_aDP = int(max_aDP)
        n = C.c_int64(0)
        rc = fn(self.h, arr, len(rows), C.byref(req), None, 0, C.byref(n))
        if rc != _ffi.ENUMS["UVCGPU_ENOMEM"]:
            self._check(rc)
        out = np.zeros(max(n.value, 1), dtype=CALLABLE_RUN)
        self._check(fn(self.h, arr, len(rows), C.byref(req), out.ctypes.data, n.value, C.byref(n)))
        return out[:n.value].copy()

    def site_reads(self, sites, min_mapq=0, alt_only=False):
        """uvcgpu_region_site_reads: the alignments of the region's reads behind `sites` -- zero-based positions, strictly ascending, inside
        the region.  -> (rows, counts): rows a structured array of SITE_READ (site: index into `sites`; read: the alignment's index in the
        reads as given; q: query index; obs: kind | quality << 8, kind of SITE_READ_KINDS; ins_q, ins_len, del_len: the InDels anchored at
        the site; reserved 0), ascending by (read, site); counts int32 [n_sites, 8]: the observations of each kind, those with an insertion
        and those with a deletion behind them, over all alignments with mapq >= min_mapq, whatever alt_only says.  alt_only keeps the rows
        that differ from the reference: a deletion, an InDel anchored at the site, or an A/C/G/T base other than an A/C/G/T reference
        symbol.  The quality is the handle's present one (after correct_bq() the corrected one); uvcgpu.h has the rules.  Found and
        compacted on the device; asks for the size first, then for the rows: the count pass runs once for the size and once more with the
        rows (a third time while the handle's report buffer still has to grow), so a caller who times the call, or who knows a bound of
        the rows, calls uvcgpu_region_site_reads itself with room (scripts/gpu_sitereads_bench.py does).  Legal where family_stats() is."""
        fn = self._ranges_fn("region_site_reads", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p])
        arr = np.ascontiguousarray(sites, dtype=np.int32)
        req = _ffi.UvcSiteReadsRequest(int(min_mapq), int(alt_only))
        counts = np.zeros((len(arr), _ffi.ENUMS["UVC_SITEREAD_NCOL"]), dtype=np.int32)
        n = C.c_int64(0)
        rc = fn(self.h, arr.ctypes.data, len(arr), C.byref(req), counts.ctypes.data, None, 0, C.byref(n))
        if rc != _ffi.ENUMS["UVCGPU_ENOMEM"]:
            self._check(rc)
        out = np.zeros(max(n.value, 1), dtype=SITE_READ)
        if n.value:
            self._check(fn(self.h, arr.ctypes.data, len(arr), C.byref(req), counts.ctypes.data, out.ctypes.data, n.value, C.byref(n)))
        return out[:n.value].copy(), counts

    def clip_sites(self, ranges, min_mapq=0, min_clip=10, min_reads=3, want_reads=False):
        """uvcgpu_region_clip_sites: the (position, side) sites inside `ranges` -- (pos_beg, pos_end) pairs as for coverage() -- at which the
        soft and hard clips of the region's reads pile up: at least min_reads alignments with mapq >= min_mapq whose clip of at least
        min_clip bases (S + H) ends there.  -> (totals, rows, reads): totals int64 [8] (_ffi.CLIPSITE_TOTALS names the first five); rows
        int64 [n_sites, UVC_CLIPSITE_ROW], sorted by (pos, side): range, pos, side (0 left, 1 right), reads, reads_fwd, reads_supp,
        reads_secondary, reads_hard, len_sum, len_max, mapq_sum, spanning and VOTE[32][5], the base votes over the clipped sequence
        counted outward from the junction (_ffi.CLIPSITE_SECTIONS names the sections, uvcgpu.h has the rules); reads: with want_reads a
        structured array of CLIP_READ (site: index into rows; read: the alignment's index in the reads as given; soft_len, hard_len), one
        per event behind a site, ascending by (read, side), else None.  Found and filled on the device; asks for the sizes first, then
        for the rows.  Legal where read_profile() is."""
        fn = self._ranges_fn("region_clip_sites", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p])
        arr, rows = _coverage_ranges(ranges)
        req = _ffi.UvcClipSitesRequest(int(min_mapq), int(min_clip), int(min_reads), int(want_reads))
        totals = np.zeros(_ffi.ENUMS["UVC_CLIPSITE_NTOTAL"], dtype=np.int64)
        ns, nr = C.c_int64(0), C.c_int64(0)
        rc = fn(self.h, arr, len(rows), C.byref(req), totals.ctypes.data, None, 0, C.byref(ns), None, 0, C.byref(nr))
        if rc != _ffi.ENUMS["UVCGPU_ENOMEM"]:
            self._check(rc)
        out = np.zeros((max(ns.value, 1), _ffi.ENUMS["UVC_CLIPSITE_ROW"]), dtype=np.int64)
        ev = np.zeros(max(nr.value, 1), dtype=CLIP_READ)
        if rc:
            self._check(fn(self.h, arr, len(rows), C.byref(req), totals.ctypes.data, out.ctypes.data, ns.value, C.byref(ns), ev.ctypes.data if want_reads else None, nr.value if want_reads else 0, C.byref(nr)))
        return totals, out[:ns.value].copy(), (ev[:nr.value].copy() if want_reads else None)

    def clip_junctions(self, rows, min_votes=2, min_len=16, max_mismatch=1, max_dist=0, mate_slop=10):
        """uvcgpu_region_clip_junctions: where the clipped consensus of each site row of clip_sites() lies on the reference of this region,
        on which strand, how unique that is and which other row is the far end of the event.  A vote index is compared when it has at
        least min_votes votes and a two-thirds A/C/G/T majority; a site is searched with at least min_len compared indices; a placement
        counts with at most max_mismatch (0..7) mismatches and, with max_dist > 0, a partner at most max_dist from the site; the mate is
        the nearest row of the expected side within mate_slop of the partner.  -> (totals, junction rows): totals int64 [8]
        (_ffi.CLIPJUNC_TOTALS names the first five); rows int64 [n_sites, UVC_CLIPJUNC_ROW]: site, query_len, cmp_len, status (0 not
        searched, 1 not placed, 2 placed), best_mm, n_best, second_mm, partner (absolute), strand (0 forward, 1 reverse), klass
        (_ffi.CLIP_CLASSES), len, mate (a row index or -1), hist[8] (_ffi.CLIPJUNC_SECTIONS names the sections, uvcgpu.h has the rules).
        A partner is found only inside this region.  Legal from the creation of the region on; reads no reads and no planes."""
        fn = self._ranges_fn("region_clip_junctions", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p])
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, _ffi.ENUMS["UVC_CLIPSITE_ROW"])
        req = _ffi.UvcClipJunctionsRequest(int(min_votes), int(min_len), int(max_mismatch), int(max_dist), int(mate_slop))
        totals = np.zeros(_ffi.ENUMS["UVC_CLIPJUNC_NTOTAL"], dtype=np.int64)
        out = np.zeros((max(len(rows), 1), _ffi.ENUMS["UVC_CLIPJUNC_ROW"]), dtype=np.int64)
        self._check(fn(self.h, rows.ctypes.data if len(rows) else None, len(rows), C.byref(req), out.ctypes.data, totals.ctypes.data))
        return totals, out[:len(rows)].copy()

    def clip_mates(self, rows, mtid, tid, min_mapq=0, window=500, overhang=5, min_dist=1000, max_gap=500, min_pairs=2, want_reads=True):
        """uvcgpu_region_clip_mates: the read pairs of the region's reads that face each site row of clip_sites() and where the mates of the
        discordant ones cluster.  mtid: the contig of every alignment's mate, one int32 per alignment in the order of the reads as given,
        or None (every mate on `tid`, the region's contig).  A forward pair read faces a RIGHT site p when pos < p and p - window < end <=
        p + overhang, a reverse one a LEFT site p when end > p and p - overhang <= pos < p + window; an item is OTHER_CONTIG, SAME_STRAND,
        FAR (|mpos - pos| >= min_dist) or CONCORDANT; the discordant ones, ordered by (site, mate contig, mate strand, mpos, read), are cut
        into clusters where the contig or strand changes or mpos grows by more than max_gap; a cluster of at least min_pairs is kept.
        -> (totals, site rows, cluster rows, reads): totals int64 [8] (_ffi.CLIPMATE_TOTALS names the first seven); site rows int64
        [n_sites, UVC_CLIPMATE_SITE_ROW] (_ffi.CLIPMATE_SITE_WORDS); cluster rows int64 [n_kept, UVC_CLIPMATE_ROW]
        (_ffi.CLIPMATE_CLUSTER_WORDS); reads: with want_reads a structured array of CLIP_MATE (site, read, cluster: index into the cluster
        rows or -1, klass: _ffi.CLIPMATE_CLASSES), one per witness in witness order, else None.  uvcgpu.h has the rules.  Gathered, ranked
        and clustered on the device; asks for the sizes first, then for the rows.  Legal where clip_sites() is."""
        fn = self._ranges_fn("region_clip_mates", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                                            C.c_void_p])
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, _ffi.ENUMS["UVC_CLIPSITE_ROW"])
        mt = None if mtid is None else np.ascontiguousarray(mtid, dtype=np.int32)
        req = _ffi.UvcClipMatesRequest(int(tid), int(min_mapq), int(window), int(overhang), int(min_dist), int(max_gap), int(min_pairs), int(want_reads))
        totals = np.zeros(_ffi.ENUMS["UVC_CLIPMATE_NTOTAL"], dtype=np.int64)
        site_rows = np.zeros((max(len(rows), 1), _ffi.ENUMS["UVC_CLIPMATE_SITE_ROW"]), dtype=np.int64)
        nc, nr = C.c_int64(0), C.c_int64(0)
        args = (self.h, rows.ctypes.data if len(rows) else None, len(rows), None if mt is None else mt.ctypes.data, C.byref(req), totals.ctypes.data, site_rows.ctypes.data)
        rc = fn(*args, None, 0, C.byref(nc), None, 0, C.byref(nr))
        if rc != _ffi.ENUMS["UVCGPU_ENOMEM"]:
            self._check(rc)
        out = np.zeros((max(nc.value, 1), _ffi.ENUMS["UVC_CLIPMATE_ROW"]), dtype=np.int64)
        ev = np.zeros(max(nr.value, 1), dtype=CLIP_MATE)
        if rc:
            self._check(fn(*args, out.ctypes.data, nc.value, C.byref(nc), ev.ctypes.data if want_reads else None, nr.value if want_reads else 0, C.byref(nr)))
        return totals, site_rows[:len(rows)].copy(), out[:nc.value].copy(), (ev[:nr.value].copy() if want_reads else None)

    def msi(self, ranges, min_tracklen=10, min_units=5, max_unitlen=6):
        """uvcgpu_region_msi: the microsatellite loci whose head lies in `ranges` -- (pos_beg, pos_end) pairs as for coverage() -- as the STR
        planes of the region name them: tracts of at least min_tracklen bp and min_units whole units of at most max_unitlen bp.  int32
        [n_loci, UVC_MSI_ROW], sorted by position: range, pos_beg, tracklen, unitlen, flags (UVC_MSI_EDGE: the tract touches an end of the
        region; nothing was counted), depth[4] (the smallest bDP, cDP12, cDP2, dDP1 along the tract) and hist[4][13] (per level the InDel
        alleles that shift the tract by -6..-1, +1..+6 whole units, then OTHER); _ffi.MSI_SECTIONS names the sections, uvcgpu.h has the
        rules.  Found and tallied on the device; asks for the size first, then for the rows.  After accumulate() and before anything that
        releases the planes."""
        fn = self._ranges_fn("region_msi", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p])
        arr, rows = _coverage_ranges(ranges)
        req = _ffi.UvcMsiRequest(int(min_tracklen), int(min_units), int(max_unitlen))
        n = C.c_int64(0)
        rc = fn(self.h, arr, len(rows), C.byref(req), None, 0, C.byref(n))
        if rc != _ffi.ENUMS["UVCGPU_ENOMEM"]:
            self._check(rc)
        out = np.zeros((max(n.value, 1), _ffi.ENUMS["UVC_MSI_ROW"]), dtype=np.int32)
        self._check(fn(self.h, arr, len(rows), C.byref(req), out.ctypes.data, n.value, C.byref(n)))
        return out[:n.value].copy()

    def score_stream_bytes_per_record(self):
        return self._ranges_fn("score_stream_bytes_per_record", C.c_int64, [])()

    def score_stream_footprint(self):
        return self._ranges_fn("score_stream_footprint", C.c_int64, [C.c_void_p])(self.h)

    def vcf_records_ranges(self, contig_name, records, ranges, tumor_keys=None, tumor_sample_columns=None, tumor_ref_alt=None):
        """uvcgpu_region_vcf_records_ranges: the text of the records score_ranges(ranges) returned = the single-range texts one after another."""
        fn = self._ranges_fn("region_vcf_records_ranges", C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(_ffi.UvcScoreOut), C.POINTER(_ffi.UvcScoreRequest), C.c_void_p, C.c_int64,
                                                                    C.c_void_p, C.c_int64, C.POINTER(C.c_int64)])
        n = len(records["refpos"])
        buf = np.ascontiguousarray(np.stack([np.asarray(records[name], dtype=np.int32) for name in _ffi.SCORE_FIELDS])) if n else np.zeros((_ffi.NUM_SCORE_FIELDS, 1), dtype=np.int32)
        so = _ffi.UvcScoreOut(max(n, 1), n, buf.ctypes.data)
        req, _keep = self.make_request(tumor_keys=tumor_keys, tumor_sample_columns=tumor_sample_columns, tumor_ref_alt=tumor_ref_alt)
        arr, nr = self.make_ranges(ranges)
        ln = C.c_int64(0)
        rc = fn(self.h, contig_name.encode(), C.byref(so), C.byref(req), arr, nr, None, 0, C.byref(ln))
        if rc not in (0, -6):
            self._check(rc)
        dst = C.create_string_buffer(max(1, ln.value))
        self._check(fn(self.h, contig_name.encode(), C.byref(so), C.byref(req), arr, nr, dst, ln.value, C.byref(ln)))
        return dst.raw[:ln.value].decode()

    def fetch_columns(self, refpos):
        """Every plane value of the given positions (uvcgpu_region_fetch_columns): int64 [len(refpos), n_columns]; `column_base(group)`
        gives the first column of a plane group, the planes of a group follow in the order of `fetch(group)`."""
        fn = getattr(self.lib.dll, self.lib.prefix + "region_fetch_columns")
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        ncol = getattr(self.lib.dll, self.lib.prefix + "region_n_columns")
        ncol.restype, ncol.argtypes = C.c_int32, []
        pos = np.ascontiguousarray(refpos, dtype=np.int32)
        out = np.zeros((len(pos), ncol()), dtype=np.int64)
        self._check(fn(self.h, pos.ctypes.data, len(pos), out.ctypes.data))
        return out

    def column_base(self, group):
        fn = getattr(self.lib.dll, self.lib.prefix + "region_column_base")
        fn.restype, fn.argtypes = C.c_int32, [C.c_int32]
        return fn(_ffi.FIELD_GROUPS[group][0])

    def vcf_records(self, contig_name, records, tumor_keys=None, pos_beg=-1, pos_end=-1, base_at_pos_beg=False, region_beg=0, tumor_sample_columns=None, tumor_ref_alt=None):
        """The VCF lines (text) of the records `score()` returned that are written (out and keep set): uvcgpu_region_vcf_records.
        Needs the planes, i.e. a score call without release_state.  The keyword arguments repeat those of the score call."""
        fn = getattr(self.lib.dll, self.lib.prefix + "region_vcf_records")
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(_ffi.UvcScoreOut), C.POINTER(_ffi.UvcScoreRequest), C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        n = len(records["refpos"])
        buf = np.ascontiguousarray(np.stack([np.asarray(records[name], dtype=np.int32) for name in _ffi.SCORE_FIELDS])) if n else np.zeros((_ffi.NUM_SCORE_FIELDS, 1), dtype=np.int32)
        so = _ffi.UvcScoreOut(max(n, 1), n, buf.ctypes.data)
        req, _keep = self.make_request(pos_beg=pos_beg, pos_end=pos_end, tumor_keys=tumor_keys, base_at_pos_beg=base_at_pos_beg, region_beg=region_beg, tumor_sample_columns=tumor_sample_columns, tumor_ref_alt=tumor_ref_alt)
        ln = C.c_int64(0)
        rc = fn(self.h, contig_name.encode(), C.byref(so), C.byref(req), None, 0, C.byref(ln))
        if rc not in (0, -6):
            self._check(rc)
        dst = C.create_string_buffer(max(1, ln.value))
        self._check(fn(self.h, contig_name.encode(), C.byref(so), C.byref(req), dst, ln.value, C.byref(ln)))
        return dst.raw[:ln.value].decode()

    def _alloc_score_buf(self, capacity):
        """[NUM_SCORE_FIELDS][capacity] int32 in page-locked memory of the library's own (uvcgpu_host_alloc), so that the D2H of the records runs
        at PCIe speed.  Not a pinned numpy buffer: heap pages that once were the source of a pageable upload can be mapped read-only for the
        GPU and come back from the allocator as such a buffer.  Libraries without the call (the oracle) get a plain array."""
        n = _ffi.NUM_SCORE_FIELDS * capacity
        alloc = getattr(self.lib.dll, self.lib.prefix + "host_alloc", None)
        if alloc is not None and not os.environ.get("UVC_NO_PIN"):
            alloc.restype, alloc.argtypes = C.c_int, [C.POINTER(C.c_void_p), C.c_int64]
            p = C.c_void_p()
            if alloc(C.byref(p), n * 4) == 0 and p.value:
                self._score_buf_host = p
                return np.ctypeslib.as_array((C.c_int32 * n).from_address(p.value)).reshape(_ffi.NUM_SCORE_FIELDS, capacity)
        self._score_buf_host = None
        return np.empty((_ffi.NUM_SCORE_FIELDS, capacity), dtype=np.int32)

    def _free_score_buf(self):
        p = getattr(self, "_score_buf_host", None)
        self._score_buf = None
        if p is not None and p.value:
            fn = getattr(self.lib.dll, self.lib.prefix + "host_free")
            fn.restype, fn.argtypes = C.c_int, [C.c_void_p]
            fn(p)
        self._score_buf_host = None

    def close(self):
        self._free_score_buf()
        if self.h:
            self.lib.call("destroy", self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
