"""ctypes mirror of include/uvcio.h: BAM (+ BAI) and FASTA (+ .fai) readers of libuvcio.so -- the htslib calls of the reference's
ingest (sam_itr_queryi / sam_itr_next, faidx_fetch_seq; grouping.cpp:617-731, main.cpp:529-531) on zlib only."""
import ctypes as C
import os

import numpy as np

from . import _ffi


class UvcBamBatch(C.Structure):
    _fields_ = [("n_alns", C.c_int64), ("tid", C.c_void_p), ("pos", C.c_void_p), ("endpos", C.c_void_p), ("mtid", C.c_void_p), ("mpos", C.c_void_p), ("isize", C.c_void_p),
                ("flag", C.c_void_p), ("mapq", C.c_void_p), ("nm", C.c_void_p), ("l_qseq", C.c_void_p), ("n_cigar", C.c_void_p),
                ("seq_off", C.c_void_p), ("cigar_off", C.c_void_p), ("qname_off", C.c_void_p),
                ("n_bases", C.c_int64), ("bases", C.c_void_p), ("quals", C.c_void_p), ("n_cigar_ops", C.c_int64), ("cigars", C.c_void_p),
                ("n_qname_bytes", C.c_int64), ("qnames", C.c_void_p)]


_COLS = [("tid", np.int32), ("pos", np.int32), ("endpos", np.int32), ("mtid", np.int32), ("mpos", np.int32), ("isize", np.int32), ("flag", np.uint16), ("mapq", np.uint8),
         ("nm", np.int32), ("l_qseq", np.int32), ("n_cigar", np.int32), ("seq_off", np.int64), ("cigar_off", np.int64), ("qname_off", np.int64)]
_dll = None


def library_path():
    # UVCIO_LIBRARY: another build of the same library (scripts/cpu_sanitize.sh runs the reader tests on an AddressSanitizer build)
    return os.environ.get("UVCIO_LIBRARY") or os.path.join(_ffi.ROOT, "uvc_amd", "csrc", "libuvcio.so")


def dll():
    global _dll
    if _dll is None:
        if not os.path.exists(library_path()):
            raise ImportError("%s is not built: run `python -c 'import __graft_entry__ as g; g.build()'`" % library_path())
        d = C.CDLL(library_path())
        d.uvcio_last_error.restype = C.c_char_p
        d.uvcio_bam_open.argtypes = [C.POINTER(C.c_void_p), C.c_char_p]
        d.uvcio_bam_n_refs.argtypes = [C.c_void_p]
        d.uvcio_bam_ref_name.restype, d.uvcio_bam_ref_name.argtypes = C.c_char_p, [C.c_void_p, C.c_int32]
        d.uvcio_bam_ref_len.restype, d.uvcio_bam_ref_len.argtypes = C.c_int64, [C.c_void_p, C.c_int32]
        d.uvcio_bam_has_index.argtypes = [C.c_void_p]
        d.uvcio_bam_fetch.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.POINTER(UvcBamBatch)]
        d.uvcio_bam_close.argtypes = [C.c_void_p]
        d.uvcio_fasta_open.argtypes = [C.POINTER(C.c_void_p), C.c_char_p]
        d.uvcio_fasta_seq_len.restype, d.uvcio_fasta_seq_len.argtypes = C.c_int64, [C.c_void_p, C.c_char_p]
        d.uvcio_fasta_fetch.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.c_int64, C.c_char_p]
        d.uvcio_fasta_close.argtypes = [C.c_void_p]
        d.uvcio_bam_region_bytes.restype, d.uvcio_bam_region_bytes.argtypes = C.c_int64, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64]
        d.uvcio_plan_shards.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
        d.uvcio_bgzf_concat.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_int32]
        d.uvcio_tumor_vcf_open.argtypes = [C.POINTER(C.c_void_p), C.c_char_p, C.POINTER(C.c_char_p), C.c_int32, C.c_int32]
        d.uvcio_tumor_vcf_create.argtypes = [C.POINTER(C.c_void_p), C.c_char_p, C.POINTER(C.c_char_p), C.c_int32, C.c_int32]
        d.uvcio_tumor_vcf_add_lines.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        d.uvcio_tumor_vcf_sample_name.restype, d.uvcio_tumor_vcf_sample_name.argtypes = C.c_char_p, [C.c_void_p]
        d.uvcio_tumor_vcf_n_records.restype, d.uvcio_tumor_vcf_n_records.argtypes = C.c_int64, [C.c_void_p]
        d.uvcio_tumor_vcf_fetch.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
        d.uvcio_tumor_vcf_close.argtypes = [C.c_void_p]
        d.uvcio_sites_open.argtypes = [C.POINTER(C.c_void_p), C.c_char_p, C.POINTER(C.c_char_p), C.c_int32]
        d.uvcio_sites_count.restype, d.uvcio_sites_count.argtypes = C.c_int64, [C.c_void_p]
        d.uvcio_sites_fetch.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
        d.uvcio_sites_close.argtypes = [C.c_void_p]
        _dll = d
    return _dll


def _check(rc):
    if rc != 0:
        raise IOError("uvcio error %d: %s" % (rc, dll().uvcio_last_error().decode()))


class _Names:
    """read names of a batch, decoded on demand (a list of two million Python strings is the slowest part of a fetch)"""

    def __init__(self, raw, off):
        self.raw, self.off = raw, off

    def __len__(self):
        return len(self.off)

    def __getitem__(self, i):
        o = int(self.off[i])
        return self.raw[o:self.raw.index(b"\0", o)].decode()

    def __iter__(self):
        return (self[i] for i in range(len(self)))


class Bam:
    def __init__(self, path):
        self.h = C.c_void_p()
        _check(dll().uvcio_bam_open(C.byref(self.h), path.encode()))
        self.refs = [(dll().uvcio_bam_ref_name(self.h, i).decode(), dll().uvcio_bam_ref_len(self.h, i)) for i in range(dll().uvcio_bam_n_refs(self.h))]
        self.has_index = bool(dll().uvcio_bam_has_index(self.h))

    def tid(self, name):
        return [n for n, _ in self.refs].index(name)

    def fetch(self, tid, beg, end):
        """Alignments overlapping [beg, end) of reference `tid`, in file order: dict of numpy columns (copies) + the read names."""
        b = UvcBamBatch()
        _check(dll().uvcio_bam_fetch(self.h, tid, beg, end, C.byref(b)))
        n = b.n_alns

        def col(ptr, dt, cnt):
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dt))), shape=(cnt,)).copy() if cnt else np.zeros(0, dt)
        out = {name: col(getattr(b, name), dt, n) for name, dt in _COLS}
        out["bases"] = col(b.bases, np.uint8, b.n_bases); out["quals"] = col(b.quals, np.uint8, b.n_bases); out["cigars"] = col(b.cigars, np.uint32, b.n_cigar_ops)
        raw = C.string_at(b.qnames, b.n_qname_bytes) if b.n_qname_bytes else b""
        out["qnames_raw"] = raw                      # NUL-terminated names back to back, qname_off[i] = start of the i-th
        out["qnames"] = _Names(raw, out["qname_off"])
        out["n_alns"] = n
        return out

    def close(self):
        if self.h:
            dll().uvcio_bam_close(self.h); self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Fasta:
    def __init__(self, path):
        self.h = C.c_void_p()
        _check(dll().uvcio_fasta_open(C.byref(self.h), path.encode()))

    def seq_len(self, name):
        return dll().uvcio_fasta_seq_len(self.h, name.encode())

    def fetch(self, name, beg, end):
        buf = C.create_string_buffer(max(1, end - beg))
        _check(dll().uvcio_fasta_fetch(self.h, name.encode(), beg, end, buf))
        return buf.raw[:end - beg].decode()

    def close(self):
        if self.h:
            dll().uvcio_fasta_close(self.h); self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class UvcRegionCut(C.Structure):
    _fields_ = [("tid", C.c_int32), ("beg", C.c_int32), ("end", C.c_int32), ("flag", C.c_int32), ("batch", C.c_int32), ("n_reads", C.c_int64)]


class BgzfWriter:
    """uvcio_bgzf_write_*: the block-gzipped stream the reference writes its VCF through (main.cpp:1196-1215)."""

    def __init__(self, path, level=6):
        d = dll()
        d.uvcio_bgzf_write_open.argtypes = [C.POINTER(C.c_void_p), C.c_char_p, C.c_int32]
        d.uvcio_bgzf_write.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        d.uvcio_bgzf_write_close.argtypes = [C.c_void_p]
        self.h = C.c_void_p()
        _check(d.uvcio_bgzf_write_open(C.byref(self.h), path.encode(), level))

    def write(self, data):
        b = data.encode() if isinstance(data, str) else bytes(data)
        _check(dll().uvcio_bgzf_write(self.h, b, len(b)))

    def close(self):
        if self.h:
            h, self.h = self.h, C.c_void_p()
            _check(dll().uvcio_bgzf_write_close(h))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class _Store:
    """What the stores of the reports share: an open handle `h` of the functions uvcio_<name>_*, written by write(), closed by close()
    or at the end of a `with` block, and add_target where the store has targets.  The constructors open it; what a store takes
    (add*) is its own."""

    def _bind(self, name):
        """The library with the shared functions of uvcio_<name>_* declared; the handle is not open yet."""
        self.name, self.h = name, C.c_void_p()
        self._f("write").restype, self._f("write").argtypes = C.c_int, [C.c_void_p, C.c_char_p]
        self._f("close").restype, self._f("close").argtypes = None, [C.c_void_p]
        return dll()

    def _f(self, what):
        return getattr(dll(), "uvcio_%s_%s" % (self.name, what))

    def write(self, path):
        _check(self._f("write")(self.h, str(path).encode()))

    def close(self):
        if self.h:
            h, self.h = self.h, C.c_void_p()
            self._f("close")(h)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def add_target(self, chrom, beg, end, name=None):
        """A target, added in report order: its index (FamilyStats, Callable, Msi)."""
        f = self._f("add_target")
        f.restype, f.argtypes = C.c_int64, [C.c_void_p, C.c_char_p, C.c_int64, C.c_int64, C.c_char_p]
        t = f(self.h, chrom.encode(), int(beg), int(end), name.encode() if name else None)
        if t < 0:
            _check(int(t))
        return int(t)


class FamilyStats(_Store):
    """uvcio_famstats_*: the store behind uvc1-mi355x --family-stats-out.  Targets are added in report order; a piece is one row of
    Region.family_stats (its TARGET block goes to the target, its FIRST block to the run's sum; any thread, any order); write() makes the text."""

    def __init__(self):
        d = self._bind("famstats")
        d.uvcio_famstats_open.restype, d.uvcio_famstats_open.argtypes = C.c_int, [C.POINTER(C.c_void_p)]
        d.uvcio_famstats_add_piece.restype, d.uvcio_famstats_add_piece.argtypes = C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]
        _check(d.uvcio_famstats_open(C.byref(self.h)))

    def add_piece(self, target, row):
        import numpy as np
        row = np.ascontiguousarray(row, dtype=np.int64)
        if row.shape != (365,):
            raise ValueError("a piece is one row of Region.family_stats (365 values)")
        _check(dll().uvcio_famstats_add_piece(self.h, int(target), row.ctypes.data))



class FamilyConcordance(_Store):
    """uvcio_famconcord_*: the store behind uvc1-mi355x --family-concordance-out.  add() sums one row of Region.family_concordance (any
    thread, any order: rows of disjoint position sets add); write() makes the text."""

    def __init__(self):
        d = self._bind("famconcord")
        d.uvcio_famconcord_open.restype, d.uvcio_famconcord_open.argtypes = C.c_int, [C.POINTER(C.c_void_p)]
        d.uvcio_famconcord_add.restype, d.uvcio_famconcord_add.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
        _check(d.uvcio_famconcord_open(C.byref(self.h)))

    def add(self, row):
        import numpy as np
        row = np.ascontiguousarray(row, dtype=np.int64)
        if row.shape != (1429,):
            raise ValueError("a piece is one row of Region.family_concordance (1429 values)")
        _check(dll().uvcio_famconcord_add(self.h, row.ctypes.data))


class FragmentProfile(_Store):
    """uvcio_fragprofile_*: the store behind uvc1-mi355x --fragment-profile-out.  Targets are added in report order; add_piece takes one
    TARGET row of Region.fragment_profile for a target, add_profile sums the profile row of a call (any thread, any order); write() makes
    the text."""

    def __init__(self, min_mapq=0, short=(100, 150), long=(151, 220)):
        d = self._bind("fragprofile")
        d.uvcio_fragprofile_open.restype, d.uvcio_fragprofile_open.argtypes = C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
        d.uvcio_fragprofile_add_piece.restype, d.uvcio_fragprofile_add_piece.argtypes = C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]
        d.uvcio_fragprofile_add_profile.restype, d.uvcio_fragprofile_add_profile.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
        _check(d.uvcio_fragprofile_open(C.byref(self.h), int(min_mapq), int(short[0]), int(short[1]), int(long[0]), int(long[1])))

    def add_piece(self, target, row):
        import numpy as np
        row = np.ascontiguousarray(row, dtype=np.int64)
        if row.shape != (8,):
            raise ValueError("a piece is one TARGET row of Region.fragment_profile (8 values)")
        _check(dll().uvcio_fragprofile_add_piece(self.h, int(target), row.ctypes.data))

    def add_profile(self, profile):
        import numpy as np
        profile = np.ascontiguousarray(profile, dtype=np.int64)
        if profile.shape != (2320,):
            raise ValueError("a profile is the second result of Region.fragment_profile (2320 values)")
        _check(dll().uvcio_fragprofile_add_profile(self.h, profile.ctypes.data))


class ReadProfile(_Store):
    """uvcio_readprofile_*: the store behind uvc1-mi355x --read-profile-out.  add() sums one row of Region.read_profile (any thread, any
    order: rows of disjoint position sets add); write() makes the text."""
    add_target = None   # one row for the whole run: no targets

    def __init__(self, classes, min_mapq=0, min_depth=20, max_alt_permille=50):
        d = self._bind("readprofile")
        d.uvcio_readprofile_open.restype, d.uvcio_readprofile_open.argtypes = C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_char_p), C.c_int32, C.c_int32, C.c_int32]
        d.uvcio_readprofile_add.restype, d.uvcio_readprofile_add.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
        if len(classes) != 4:
            raise ValueError("the read classes are four (region.READ_CLASSES)")
        _check(d.uvcio_readprofile_open(C.byref(self.h), (C.c_char_p * 4)(*[c.encode() for c in classes]), int(min_mapq), int(min_depth), int(max_alt_permille)))

    def add(self, row):
        import numpy as np
        row = np.ascontiguousarray(row, dtype=np.int64)
        if row.shape != (5712,):
            raise ValueError("a piece is one row of Region.read_profile (5712 values)")
        _check(dll().uvcio_readprofile_add(self.h, row.ctypes.data))



class SiteReads(_Store):
    """uvcio_sitereads_*: the store behind uvc1-mi355x --site-reads-out.  add() takes the sites (zero-based), counts and rows of one
    Region.site_reads with the columns of that call's alignments (any thread, any order; the rows of a site come from one call); a call
    without counts lists sites that nobody reported on.  write() sorts by (contig id, position) and makes the S / A / R lines."""
    add_target = None   # the sites are the targets

    def __init__(self, kinds, classes, min_mapq=0, alt_only=True):
        d = self._bind("sitereads")
        d.uvcio_sitereads_open.restype, d.uvcio_sitereads_open.argtypes = C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_int32, C.c_int32]
        d.uvcio_sitereads_add.restype, d.uvcio_sitereads_add.argtypes = C.c_int, [C.c_void_p, C.c_int32, C.c_char_p, C.c_void_p, C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                                                                  C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        if len(kinds) != 6 or len(classes) != 4:
            raise ValueError("the kinds are six (region.SITE_READ_KINDS), the read classes four (region.READ_CLASSES)")
        _check(d.uvcio_sitereads_open(C.byref(self.h), (C.c_char_p * 6)(*[k.encode() for k in kinds]), (C.c_char_p * 4)(*[c.encode() for c in classes]), int(min_mapq), int(alt_only)))

    def add(self, tid, contig, sites, ref=None, counts=None, rows=None, reads=None, qnames=None):
        """sites: the zero-based positions of the call; ref: their reference bases as one string, or None; counts, rows: what
        Region.site_reads returned, or None for sites without a report; reads: the reads the region was given (flag, mapq, l_qseq,
        fam_id, fam_strand, frag_id, bases, seq_off); qnames: one name per alignment."""
        import numpy as np
        sites = np.ascontiguousarray(sites, dtype=np.int32)
        if ref is not None and len(ref) != len(sites):
            raise ValueError("ref holds one base per site")
        n_rows = 0 if rows is None else len(rows)
        if counts is not None:
            counts = np.ascontiguousarray(counts, dtype=np.int32)
            if counts.shape != (len(sites), 8):
                raise ValueError("counts is the second result of Region.site_reads ([n_sites, 8])")
        if n_rows == 0:
            _check(dll().uvcio_sitereads_add(self.h, int(tid), contig.encode(), sites.ctypes.data, ref.encode() if ref is not None else None, len(sites), counts.ctypes.data if counts is not None else None,
                                             None, 0, 0, None, None, None, None, None, None, None, None, None))
            return
        rows = np.ascontiguousarray(rows)
        if rows.dtype.itemsize != 32 or counts is None or reads is None or qnames is None:
            raise ValueError("rows come with the counts of their call, the reads and their names")
        n = len(qnames)
        col = lambda k, t: np.ascontiguousarray(reads[k], dtype=t)                      # noqa: E731
        fl, mq, lq, fam, st, fr, ba, so = col("flag", np.uint16), col("mapq", np.uint8), col("l_qseq", np.int32), col("fam_id", np.int32), col("fam_strand", np.uint8), col("frag_id", np.int32), col("bases", np.uint8), col("seq_off", np.int64)
        if min(len(fl), len(mq), len(lq), len(fam), len(st), len(fr), len(so)) < n:
            raise ValueError("every alignment has a name")
        names = (C.c_char_p * n)(*[q.encode() if isinstance(q, str) else q for q in qnames])
        _check(dll().uvcio_sitereads_add(self.h, int(tid), contig.encode(), sites.ctypes.data, ref.encode() if ref is not None else None, len(sites), counts.ctypes.data, rows.ctypes.data, n_rows, n,
                                         names, fl.ctypes.data, mq.ctypes.data, lq.ctypes.data, fam.ctypes.data, st.ctypes.data, fr.ctypes.data, ba.ctypes.data, so.ctypes.data))


class ClipSites(_Store):
    """uvcio_clipsites_*: the store behind uvc1-mi355x --clip-sites-out.  add() takes the site rows and event rows of one
    Region.clip_sites(want_reads=True) with the columns of that call's alignments (any thread, any order; a site comes from one call).
    write() sorts by (contig id, position, side) and makes the S lines, with_reads the R lines behind them."""
    add_target = None   # the sites are found, not given

    def __init__(self, min_mapq=0, min_clip=10, min_reads=3, with_reads=False):
        d = self._bind("clipsites")
        d.uvcio_clipsites_open.restype, d.uvcio_clipsites_open.argtypes = C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int32, C.c_int32]
        d.uvcio_clipsites_add.restype, d.uvcio_clipsites_add.argtypes = C.c_int, [C.c_void_p, C.c_int32, C.c_char_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64,
                                                                                  C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        d.uvcio_clipsites_set_junctions.restype, d.uvcio_clipsites_set_junctions.argtypes = C.c_int, [C.c_void_p] + [C.c_int32] * 5
        d.uvcio_clipsites_add_junctions.restype, d.uvcio_clipsites_add_junctions.argtypes = C.c_int, [C.c_void_p, C.c_int32, C.c_char_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64,
                                                                                                      C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        d.uvcio_clipsites_set_mates.restype, d.uvcio_clipsites_set_mates.argtypes = C.c_int, [C.c_void_p] + [C.c_int32] * 5 + [C.POINTER(C.c_char_p), C.c_int32]
        d.uvcio_clipsites_add_mates.restype, d.uvcio_clipsites_add_mates.argtypes = C.c_int, d.uvcio_clipsites_add_junctions.argtypes + [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
        _check(d.uvcio_clipsites_open(C.byref(self.h), int(min_mapq), int(min_clip), int(min_reads), int(with_reads)))

    def set_junctions(self, min_votes=2, min_len=16, max_mismatch=1, max_dist=0, mate_slop=10):
        """Turns the J lines on: the request values of the Region.clip_junctions calls whose rows add(junctions=) hands over."""
        _check(dll().uvcio_clipsites_set_junctions(self.h, int(min_votes), int(min_len), int(max_mismatch), int(max_dist), int(mate_slop)))

    def set_mates(self, window=500, overhang=5, min_dist=1000, max_gap=500, min_pairs=2, contig_names=()):
        """Turns the P and M lines on: the request values of the Region.clip_mates calls whose results add(mates=) hands over, and the
        contig names of the BAM header, which the mate contig ids index."""
        names = (C.c_char_p * max(len(contig_names), 1))(*[c.encode() if isinstance(c, str) else c for c in contig_names])
        _check(dll().uvcio_clipsites_set_mates(self.h, int(window), int(overhang), int(min_dist), int(max_gap), int(min_pairs), names, len(contig_names)))

    def add(self, tid, contig, rows, events=None, reads=None, qnames=None, junctions=None, mates=None):
        """rows, events: the second and third result of Region.clip_sites; reads: the reads the region was given (flag, mapq, fam_id,
        fam_strand, frag_id); qnames: one name per alignment; junctions: the second result of Region.clip_junctions(rows), or None; mates:
        the second, third and fourth result of Region.clip_mates(rows, ..., want_reads=True) -- (site rows, cluster rows, reads) -- or None."""
        import numpy as np
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        if rows.ndim != 2 or rows.shape[1] != 176:
            raise ValueError("rows is the second result of Region.clip_sites ([n_sites, 176])")
        if junctions is not None:
            junctions = np.ascontiguousarray(junctions, dtype=np.int64)
            if junctions.shape != (len(rows), 24):
                raise ValueError("junctions is the second result of Region.clip_junctions(rows) ([n_sites, 24])")
        jp = junctions.ctypes.data if junctions is not None and len(rows) else None
        mate_args = (None, None, 0, None, 0)
        n_wit = 0
        if mates is not None:
            msites, mclus, mwit = (np.ascontiguousarray(mates[0], dtype=np.int64), np.ascontiguousarray(mates[1], dtype=np.int64), np.ascontiguousarray(mates[2]))
            if msites.shape != (len(rows), 8) or mclus.ndim != 2 or mclus.shape[1] != 12 or mwit.dtype.itemsize != 16:
                raise ValueError("mates is (site rows [n_sites, 8], cluster rows [n, 12], reads) of Region.clip_mates(rows, ..., want_reads=True)")
            n_wit = len(mwit)
            if len(rows):
                mate_args = (msites.ctypes.data, mclus.ctypes.data if len(mclus) else None, len(mclus), mwit.ctypes.data if n_wit else None, n_wit)
        n_ev = 0 if events is None else len(events)
        if n_ev == 0 and n_wit == 0:
            _check(dll().uvcio_clipsites_add_mates(self.h, int(tid), contig.encode(), rows.ctypes.data, jp, len(rows), None, 0, 0, None, None, None, None, None, None, *mate_args))
            return
        if reads is None or (n_ev and qnames is None):
            raise ValueError("event rows come with the reads of their call and their names, witness rows with the reads of their call")
        ep = None
        if n_ev:
            events = np.ascontiguousarray(events)
            if events.dtype.itemsize != 16:
                raise ValueError("event rows come with the reads of their call and their names")
            ep = events.ctypes.data
        col = lambda k, t: np.ascontiguousarray(reads[k], dtype=t)                      # noqa: E731
        fl, mq, fam, st, fr = col("flag", np.uint16), col("mapq", np.uint8), col("fam_id", np.int32), col("fam_strand", np.uint8), col("frag_id", np.int32)
        n = len(qnames) if qnames is not None else min(len(fl), len(mq), len(fam), len(st), len(fr))
        if min(len(fl), len(mq), len(fam), len(st), len(fr)) < n:
            raise ValueError("every alignment has a name")
        names = (C.c_char_p * n)(*[q.encode() if isinstance(q, str) else q for q in qnames]) if qnames is not None else None
        _check(dll().uvcio_clipsites_add_mates(self.h, int(tid), contig.encode(), rows.ctypes.data, jp, len(rows), ep, n_ev, n, names, fl.ctypes.data, mq.ctypes.data, fam.ctypes.data, st.ctypes.data,
                                               fr.ctypes.data, *mate_args))


class Callable(_Store):
    """uvcio_callable_*: the store behind uvc1-mi355x --callable-out.  Targets are added in report order with their positions inside the
    contig; add_runs takes the runs of one Region.callable and the target of each of its ranges (any thread, any order); write() sorts,
    fills what no piece reported with the mask of depth 0, joins equal neighbours inside a target and makes the BED text."""

    def __init__(self, measures, min_depth, max_aDP, bits):
        d = self._bind("callable")
        d.uvcio_callable_open.restype, d.uvcio_callable_open.argtypes = C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_char_p), C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_char_p), C.c_int32]
        d.uvcio_callable_add_runs.restype, d.uvcio_callable_add_runs.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
        d.uvcio_callable_n_runs.restype, d.uvcio_callable_n_runs.argtypes = C.c_int64, [C.c_void_p]
        names = (C.c_char_p * len(measures))(*[m.encode() for m in measures])
        bnames = (C.c_char_p * len(bits))(*[b.encode() for b in bits])
        md = (C.c_int32 * len(measures))(*[int(v) for v in min_depth])
        _check(d.uvcio_callable_open(C.byref(self.h), names, len(measures), md, int(max_aDP), bnames, len(bits)))

    def add_runs(self, target_of_range, runs):
        """runs: the structured array of Region.callable (range, pos_beg, pos_end, mask); target_of_range[k]: the target of the call's range k"""
        import numpy as np
        runs = np.ascontiguousarray(runs)
        if runs.dtype.itemsize != 16:
            raise ValueError("runs are the 16-byte rows of Region.callable")
        tor = np.ascontiguousarray(target_of_range, dtype=np.int64)
        _check(dll().uvcio_callable_add_runs(self.h, tor.ctypes.data, len(tor), runs.ctypes.data, len(runs)))

    def n_runs(self):
        return int(dll().uvcio_callable_n_runs(self.h))



class Msi(_Store):
    """uvcio_msi_*: the store behind uvc1-mi355x --msi-out.  Targets are added in report order with their positions inside the contig; add
    takes the rows of one Region.msi, the target of each of its ranges and the first unit of each locus as text (any thread, any order);
    write() sorts by target then position and makes the tab-separated text with its #summary lines."""

    def __init__(self, min_tracklen=10, min_units=5, max_unitlen=6, min_depth=30, unstable_permille=200):
        d = self._bind("msi")
        d.uvcio_msi_open.restype, d.uvcio_msi_open.argtypes = C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
        d.uvcio_msi_add.restype, d.uvcio_msi_add.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_char_p), C.c_int64]
        d.uvcio_msi_n_loci.restype, d.uvcio_msi_n_loci.argtypes = C.c_int64, [C.c_void_p]
        _check(d.uvcio_msi_open(C.byref(self.h), int(min_tracklen), int(min_units), int(max_unitlen), int(min_depth), int(unstable_permille)))

    def add(self, target_of_range, loci, units):
        """loci: the int32 [n][UVC_MSI_ROW] array of Region.msi; units[k]: the reference bases of the first unit of locus k;
        target_of_range[k]: the target of the call's range k"""
        import numpy as np
        loci = np.ascontiguousarray(loci, dtype=np.int32)
        if loci.ndim != 2 or len(units) != len(loci):
            raise ValueError("loci are the rows of Region.msi, one unit text each")
        tor = np.ascontiguousarray(target_of_range, dtype=np.int64)
        texts = (C.c_char_p * max(len(units), 1))(*[u.encode() for u in units])
        _check(dll().uvcio_msi_add(self.h, tor.ctypes.data, len(tor), loci.ctypes.data, texts, len(loci)))

    def n_loci(self):
        return int(dll().uvcio_msi_n_loci(self.h))



def plan_regions(tid, pos, endpos, flag, target_lens, nthreads=1, mem_per_thread_mb=1536):
    """SamIter::iternext without a BED file (grouping.cpp:225-312) over alignment columns in file order: the blocks the reference hands
    to process_batch, as dicts (tid, beg, end, flag, batch, n_reads)."""
    d = dll()
    d.uvcio_plan_regions.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    a = [np.ascontiguousarray(tid, dtype=np.int32), np.ascontiguousarray(pos, dtype=np.int32), np.ascontiguousarray(endpos, dtype=np.int32), np.ascontiguousarray(flag, dtype=np.uint16)]
    tl = np.ascontiguousarray(target_lens, dtype=np.int64)
    n = C.c_int64(0)
    rc = d.uvcio_plan_regions(a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, len(a[0]), tl.ctypes.data, len(tl), nthreads, mem_per_thread_mb, None, 0, C.byref(n))
    if rc not in (0, -6):
        _check(rc)
    out = (UvcRegionCut * max(1, n.value))()
    _check(d.uvcio_plan_regions(a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, len(a[0]), tl.ctypes.data, len(tl), nthreads, mem_per_thread_mb, out, n.value, C.byref(n)))
    return [dict(tid=c.tid, beg=c.beg, end=c.end, flag=c.flag, batch=c.batch, n_reads=c.n_reads) for c in out[:n.value]]


class UvcBedPiece(C.Structure):
    _fields_ = [("line", C.c_int64), ("batch", C.c_int64), ("beg", C.c_int64), ("end", C.c_int64)]


def plan_bed_batches(tid, beg, end, merge_distance, max_span=1000000):
    """uvcio_plan_bed_batches: BED lines (tid, beg, end) in file order -> one dict (line, batch, tid, beg, end) per line, or per piece of a
    line longer than max_span; consecutive pieces with one `batch` value become one device region (uvc1-mi355x --merge-regions)."""
    d = dll()
    d.uvcio_plan_bed_batches.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    a = [np.ascontiguousarray(tid, dtype=np.int32), np.ascontiguousarray(beg, dtype=np.int64), np.ascontiguousarray(end, dtype=np.int64)]
    n = C.c_int64(0)
    rc = d.uvcio_plan_bed_batches(a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, len(a[0]), int(merge_distance), int(max_span), None, 0, C.byref(n))
    if rc not in (0, -6):
        _check(rc)
    out = (UvcBedPiece * max(1, n.value))()
    _check(d.uvcio_plan_bed_batches(a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, len(a[0]), int(merge_distance), int(max_span), out, n.value, C.byref(n)))
    return [dict(line=int(p.line), batch=int(p.batch), tid=int(a[0][p.line]), beg=int(p.beg), end=int(p.end)) for p in out[:n.value]]


def plan_regions_stream(tid, pos, endpos, flag, target_lens, nthreads=1, mem_per_thread_mb=1536, piece=1000):
    """The same cuts through the streaming form (uvcio_planner_*): the columns are fed `piece` alignments at a time, cuts are taken as they appear."""
    d = dll()
    d.uvcio_planner_open.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_int32, C.c_int32, C.c_int64]
    d.uvcio_planner_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    d.uvcio_planner_finish.argtypes = [C.c_void_p]
    d.uvcio_planner_take.restype, d.uvcio_planner_take.argtypes = C.c_int64, [C.c_void_p, C.c_void_p, C.c_int64]
    d.uvcio_planner_close.restype, d.uvcio_planner_close.argtypes = None, [C.c_void_p]
    a = [np.ascontiguousarray(tid, dtype=np.int32), np.ascontiguousarray(pos, dtype=np.int32), np.ascontiguousarray(endpos, dtype=np.int32), np.ascontiguousarray(flag, dtype=np.uint16)]
    tl = np.ascontiguousarray(target_lens, dtype=np.int64)
    h = C.c_void_p()
    _check(d.uvcio_planner_open(C.byref(h), tl.ctypes.data, len(tl), nthreads, mem_per_thread_mb))
    cuts, buf = [], (UvcRegionCut * 64)()

    def take():
        while True:
            k = d.uvcio_planner_take(h, buf, 64)
            cuts.extend(dict(tid=c.tid, beg=c.beg, end=c.end, flag=c.flag, batch=c.batch, n_reads=c.n_reads) for c in buf[:k])
            if k < 64:
                break
    try:
        for i in range(0, len(a[0]), max(1, piece)):
            s = [x[i:i + piece] for x in a]
            _check(d.uvcio_planner_feed(h, s[0].ctypes.data, s[1].ctypes.data, s[2].ctypes.data, s[3].ctypes.data, len(s[0])))
            take()
        _check(d.uvcio_planner_finish(h))
        take()
    finally:
        d.uvcio_planner_close(h)
    return cuts


class Sites:
    """Force-output sites from a BED or a VCF(.gz) (uvcio_sites_*, what uvc1-mi355x --force-sites reads): per contig the sorted, unique
    zerobased_pos values, each the VCF POS of the records it selects.  `contig_names`: the BAM header's, in tid order."""

    def __init__(self, path, contig_names):
        self.h = C.c_void_p()
        names = (C.c_char_p * max(1, len(contig_names)))(*[n.encode() for n in contig_names])
        _check(dll().uvcio_sites_open(C.byref(self.h), path.encode(), names, len(contig_names)))
        self.n_sites = dll().uvcio_sites_count(self.h)

    def fetch(self, tid, pos_beg=0, pos_end=2**31):
        """-> int32 array: the sites of `tid` with pos_beg <= site < pos_end, ascending."""
        p, n = C.c_void_p(), C.c_int64(0)
        _check(dll().uvcio_sites_fetch(self.h, tid, pos_beg, pos_end, C.byref(p), C.byref(n)))
        if n.value == 0:
            return np.zeros(0, np.int32)
        return np.ctypeslib.as_array((C.c_int32 * n.value).from_address(p.value)).copy()

    def close(self):
        if self.h:
            dll().uvcio_sites_close(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TumorVcf:
    """The tumor VCF of a T/N pair as the normal pass reads it (uvcio_tumor_vcf_*: rescue_variants_from_vcf, main.cpp:183-398)."""

    def __init__(self, path, contig_names, is_tumor_format_retrieved=True):
        self.h = C.c_void_p()
        names = (C.c_char_p * max(1, len(contig_names)))(*[n.encode() for n in contig_names])
        _check(dll().uvcio_tumor_vcf_open(C.byref(self.h), path.encode(), names, len(contig_names), int(is_tumor_format_retrieved)))
        self.sample = dll().uvcio_tumor_vcf_sample_name(self.h).decode()
        self.n_records = dll().uvcio_tumor_vcf_n_records(self.h)

    @classmethod
    def create(cls, sample, contig_names, is_tumor_format_retrieved=True):
        """An empty in-memory store (uvcio_tumor_vcf_create): the tumor pass's record lines go in by add_lines, without a file."""
        self = cls.__new__(cls)
        self.h = C.c_void_p()
        names = (C.c_char_p * max(1, len(contig_names)))(*[n.encode() for n in contig_names])
        _check(dll().uvcio_tumor_vcf_create(C.byref(self.h), sample.encode(), names, len(contig_names), int(is_tumor_format_retrieved)))
        self.sample = dll().uvcio_tumor_vcf_sample_name(self.h).decode()
        self.n_records = 0
        return self

    def add_lines(self, text):
        """Record lines of any number of tiles (str or bytes); records of one key keep the order of their adds."""
        b = text.encode() if isinstance(text, str) else bytes(text)
        _check(dll().uvcio_tumor_vcf_add_lines(self.h, b, len(b)))
        self.n_records = dll().uvcio_tumor_vcf_n_records(self.h)

    def fetch(self, tid, pos_beg, pos_end):
        """-> (ctypes array of UvcTumorKey or None, list of sample-column strings): the records with pos_beg <= symbolpos <= pos_end;
        `last_ref_alt` holds their "REF\tALT" strings."""
        keys, cols, ras, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int64(0)
        _check(dll().uvcio_tumor_vcf_fetch(self.h, tid, pos_beg, pos_end, C.byref(keys), C.byref(cols), C.byref(ras), C.byref(n)))
        self.last_ref_alt = []
        if n.value == 0:
            return None, []
        arr = (_ffi.UvcTumorKey * n.value).from_buffer_copy((_ffi.UvcTumorKey * n.value).from_address(keys.value))   # a store reuses its buffers at the next fetch
        texts = [s.decode() for s in (C.c_char_p * n.value).from_address(cols.value)]
        self.last_ref_alt = [s.decode() for s in (C.c_char_p * n.value).from_address(ras.value)]   # "REF\tALT" of the same records
        return arr, texts

    def close(self):
        if self.h:
            dll().uvcio_tumor_vcf_close(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
