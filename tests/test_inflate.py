"""BGZF inflate on the device (uvc_amd/csrc/uvc_inflate.hip, include/uvcgpu.h: uvcgpu_bgzf_inflate) against zlib.
CPU part: the decoder core (uvc_inflate_core.h, the body of the GPU thread) compiled for the host by tests/native/inflate_core_host.cpp.
Two sources of streams: zlib's own compressor (payloads) and tests/deflate_streams.py, which writes what other compressors may and zlib's
never does; zlib's inflater is the reference for both."""
import ctypes
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import deflate_streams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def payloads():
    """(name, uncompressed bytes, raw DEFLATE stream) over the block types and code shapes zlib can produce"""
    rng = np.random.default_rng(1)
    out = []
    for n in (0, 1, 2, 10, 100, 1000, 0xff00):
        datas = {"random": bytes(rng.integers(0, 256, n, dtype=np.uint8)), "2bit": bytes(rng.integers(0, 4, n, dtype=np.uint8)),
                 "periodic": (b"ACGTTGCA" * (n // 8 + 1))[:n], "reads": bytes(rng.choice(np.frombuffer(b"ACGT!#$%&IIIIFFFF", np.uint8), n))}
        for dn, data in datas.items():
            for level, strategy in ((0, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY),
                                    (6, zlib.Z_FIXED), (6, zlib.Z_HUFFMAN_ONLY), (6, zlib.Z_RLE)):
                c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
                out.append(("%s_%d_l%d_s%d" % (dn, n, level, strategy), data, c.compress(data) + c.flush()))
    return out


@pytest.fixture(scope="module")
def host_core(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("native") / "inflate_core_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "native", "inflate_core_host.cpp")])
    dll = ctypes.CDLL(so)
    dll.inflate_core_host.restype = ctypes.c_int
    dll.inflate_core_host.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32]
    dll.inflate_core_host_10_9.restype = ctypes.c_int
    dll.inflate_core_host_10_9.argtypes = dll.inflate_core_host.argtypes
    return dll


GUARD = 64


def zlib_accepts(comp, want):
    """the reference's verdict on a catalogue stream: exactly these bytes, the final block seen, nothing behind it"""
    d = zlib.decompressobj(-15)
    return d.decompress(comp) == want and d.eof and d.unused_data == b""


@pytest.fixture(scope="module")
def catalogue():
    """tests/deflate_streams.py's valid streams, each first passed by zlib's inflater: a stream zlib refuses is a bug of the builder, not a case"""
    cases = deflate_streams.catalogue()
    for c in cases:
        assert zlib_accepts(c.comp, c.out), c.name
    return cases


def core_widths(dll):
    return (("9/7", dll.inflate_core_host), ("10/9", dll.inflate_core_host_10_9))


def run_core(fn, comp, isize):
    """the core on one stream with a guard behind the output: (return code, the ISIZE bytes, guard untouched)"""
    out = np.full(isize + GUARD, 0xAB, np.uint8)
    rc = fn(comp, len(comp), out.ctypes.data, isize)
    return rc, out[:isize].tobytes(), bool((out[isize:] == 0xAB).all())


def test_catalogue_reaches_what_zlibs_compressor_does_not(catalogue):
    """the properties the catalogue is there for, read back from the streams themselves"""
    by_name = {c.name: c for c in catalogue}
    assert len(catalogue) == 44 and len(deflate_streams.invalid_catalogue()) == 20                       # an entry dropped by a later edit is noticed
    assert [c.name for c in catalogue if c.single_ll_code] == ["stored_then_eob_only_dynamic"]
    assert by_name["only_empty_fixed"].comp == b"\x03\x00" and by_name["only_empty_stored"].comp == b"\x01\x00\x00\xff\xff"
    assert len(by_name["stored_ff00"].out) == 0xff00 and max(len(c.out) for c in catalogue) <= 0xff00 and max(len(c.comp) for c in catalogue) < 0x10000
    # (that the deep streams use 15-bit members of both codes, that stored blocks start inside a byte and that header repeats cross the
    # alphabets is asserted by the builder where it makes them; that zlib decodes every stream to the builder's bytes, by the fixture)
    assert len(by_name["all_symbols_depth15"].out) > 32768 + 3000          # room for distance 32768 behind the literals


def test_decoder_core_on_the_host_equals_zlib_on_the_catalogue(host_core, catalogue):
    """uvc_inflate_core.h's lane form at the table widths of the lane kernel (9/7) and of the wave kernels (10/9): return code 0, zlib's
    bytes, and nothing written behind ISIZE"""
    for width, fn in core_widths(host_core):
        for c in catalogue:
            rc, got, guard_ok = run_core(fn, c.comp, len(c.out))
            assert rc == 0, (width, c.name, rc)
            assert got == c.out, (width, c.name)
            assert guard_ok, (width, c.name)


def test_decoder_core_refuses_structured_invalid_streams(host_core):
    """one broken rule per stream (tests/deflate_streams.py: invalid_catalogue): zlib refuses it, the core returns the error of THAT rule
    (refused for another reason, say a missed ISIZE behind an unchecked symbol, the rule would be untested), the guard stays.
    Three of them are legal streams that miss ISIZE, which zlib's inflater is not told: there the reference is the length it returns."""
    cases = deflate_streams.invalid_catalogue()
    for c in cases:
        if c.zlib_raises:
            with pytest.raises(zlib.error):
                zlib.decompress(c.comp, -15)
        else: assert len(zlib.decompress(c.comp, -15)) != c.isize, c.name
        for width, fn in core_widths(host_core):
            rc, _, guard_ok = run_core(fn, c.comp, c.isize)
            assert rc == c.core_rc, (width, c.name, rc)
            assert guard_ok, (width, c.name)


def test_decoder_core_is_more_lenient_than_zlib_in_two_places(host_core):
    """Pinned, not endorsed as DEFLATE: the core builds its tables from any code that is not over-subscribed, so an incomplete
    literal/length code decodes as long as the stream uses only codes that exist; and it stops at the final block's end without looking at
    what follows.  Both are left as they are: every BGZF block's CRC-32 is checked by the reader on the decoded bytes (uvc_io.cpp:
    inflate_block), and that is the judge of a block, for this decoder as for zlib.  What the first leniency must not open is a decode
    that runs off the incomplete code: the stream that uses one of the codes nobody has, in front of an end-of-block code and with the
    ISIZE it would otherwise meet, ends with UVC_INFL_ECODE at that code (the fast table's empty entry, then the bit-by-bit walk that
    finds no symbol)."""
    (n1, incomplete, out1), (n2, trailing, out2) = deflate_streams.lenient_catalogue()
    with pytest.raises(zlib.error):
        zlib.decompress(incomplete, -15)
    d = zlib.decompressobj(-15)
    assert d.decompress(trailing) == out2 and d.eof and d.unused_data == b"\x00\x7f\xff"     # zlib stops there too, and says what it left
    unassigned = {c.name: c for c in deflate_streams.invalid_catalogue()}["unassigned_code_of_an_incomplete_code"]
    assert unassigned.isize == len(out1) and unassigned.comp[:12] == incomplete[:12] and len(unassigned.comp) == len(incomplete) + 1   # the same header; two more bits
    for width, fn in core_widths(host_core):
        for name, comp, want in ((n1, incomplete, out1), (n2, trailing, out2)):
            rc, got, guard_ok = run_core(fn, comp, len(want))
            assert rc == 0 and got == want and guard_ok, (width, name, rc)
        rc, _, guard_ok = run_core(fn, unassigned.comp, unassigned.isize)
        assert rc == deflate_streams.ECODE and guard_ok, (width, rc)


def test_decoders_run_clean_under_address_and_undefined_sanitizers(tmp_path):
    """tests/native/inflate_sanitize_main.cpp (both widths of the core and the host fast decoder, on heap buffers of exactly the stream's and
    ISIZE's size) built with -fsanitize=address,undefined and run as a child process on the catalogue, the invalid streams and the two
    lenient ones (the stream that uses an unassigned code of an incomplete code is among the invalid): no report, and the program's own comparison with the expected bytes passes."""
    exe = str(tmp_path / "inflate_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "inflate_sanitize_main.cpp")])
    records = [(1 if c.single_ll_code else 0, c.name, c.comp, len(c.out), c.out) for c in deflate_streams.catalogue()]
    records += [(2, c.name, c.comp, c.isize, b"") for c in deflate_streams.invalid_catalogue()]
    records += [(1 if name == "incomplete_literal_code" else 0, name, comp, len(want), want) for name, comp, want in deflate_streams.lenient_catalogue()]   # (the fast decoder declines an incomplete code)
    blob = b"UVCINFL1" + struct.pack("<I", len(records))
    for kind, name, comp, isize, want in records:
        blob += struct.pack("<5I", kind, len(name), len(comp), isize, len(want)) + name.encode() + comp + want
    path = str(tmp_path / "cases.bin")
    open(path, "wb").write(blob)
    # (leak detection is off although the program frees what it allocates: LeakSanitizer stops the world with ptrace at exit, which
    # containers commonly deny, and it then fails the run; reads and writes out of bounds and undefined behaviour are what this run is for)
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stdout
    assert "%d cases, 0 failures, fast decoder declined 2" % len(records) in r.stdout, r.stdout


def test_decoder_core_on_the_host_equals_zlib(host_core):
    for name, data, comp in payloads():
        out = np.zeros(max(1, len(data)), np.uint8)
        assert host_core.inflate_core_host(comp, len(comp), out.ctypes.data, len(data)) == 0, name
        assert out[:len(data)].tobytes() == data, name


def test_decoder_core_flags_corrupt_streams(host_core):
    rng = np.random.default_rng(3)
    data = bytes(rng.integers(0, 8, 5000, dtype=np.uint8))
    c = zlib.compressobj(6, zlib.DEFLATED, -15); comp = c.compress(data) + c.flush()
    out = np.zeros(6000, np.uint8)
    for i in range(0, len(comp), 5):                  # a flipped byte anywhere: an error code or other bytes, never a crash or a silent match
        b = bytearray(comp); b[i] ^= 0x55
        rc = host_core.inflate_core_host(bytes(b), len(b), out.ctypes.data, 5000)
        assert rc != 0 or out[:5000].tobytes() != data, i
    assert host_core.inflate_core_host(comp[:len(comp) // 2], len(comp) // 2, out.ctypes.data, 5000) != 0     # truncated input
    assert host_core.inflate_core_host(comp, len(comp), out.ctypes.data, 4000) != 0                            # ISIZE too small
    assert host_core.inflate_core_host(comp, len(comp), out.ctypes.data, 6000) != 0                            # ISIZE too large


def _gpu_inflate(lib, comps, sizes):
    fn = lib.dll.uvcgpu_bgzf_inflate
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64]
    comp = np.frombuffer(b"".join(comps) + b"\0" * 8, np.uint8).copy()
    in_len = np.array([len(c) for c in comps], np.int32); in_off = np.concatenate([[0], np.cumsum(in_len[:-1])]).astype(np.int64)
    out_len = np.array(sizes, np.int32); out_off = (np.concatenate([[0], np.cumsum(out_len[:-1])]) + 100).astype(np.int64)   # the first 100 bytes are the caller's
    out = np.full(int(out_len.sum()) + 200, 0xAB, np.uint8)
    rc = fn(None, comp.ctypes.data, len(comp), in_off.ctypes.data, in_len.ctypes.data, out_off.ctypes.data, out_len.ctypes.data, len(comps), out.ctypes.data, len(out))
    return rc, out, out_off


@pytest.fixture(params=["lane per block", "wave per block", "wave per block, 8 waves per SIMD"])
def kernel_form(request, monkeypatch):
    """uvc_inflate.hip has three kernels, chosen by UVCGPU_INFLATE_WAVE at every call: 0 k_bgzf_inflate, 1 k_bgzf_inflate_wave, 8 (default) k_bgzf_inflate_wave8"""
    if request.param.startswith("wave per block"): monkeypatch.setenv("UVCGPU_INFLATE_WAVE", "8" if "8" in request.param else "1")
    else: monkeypatch.setenv("UVCGPU_INFLATE_WAVE", "0")
    return request.param


@pytest.mark.gpu
def test_device_inflate_equals_zlib(gpu_lib, kernel_form):
    cases = payloads()
    rc, out, off = _gpu_inflate(gpu_lib, [c for _, _, c in cases], [len(d) for _, d, _ in cases])
    assert rc == 0, gpu_lib.last_error()
    for (name, data, _), o in zip(cases, off):
        assert out[o:o + len(data)].tobytes() == data, name
    total = sum(len(d) for _, d, _ in cases)
    assert (out[:100] == 0xAB).all() and (out[100 + total:] == 0xAB).all()          # nothing outside the blocks' range is written


@pytest.mark.gpu
def test_device_inflate_of_a_bam_and_a_corrupt_block(gpu_lib, tmp_path, kernel_form):
    import bamwriter
    from uvc_amd import synth
    reads = synth.generate_region(seed=77, region_len=20000, depth=200)
    path = str(tmp_path / "t.bam")
    bamwriter.write_bam(path, [("chrT", int(reads["end"]) + 1000)], bamwriter.records_from_reads(reads))
    raw = open(path, "rb").read()
    comps, sizes, want = [], [], []
    off = 0
    while off + 18 <= len(raw):
        bsize = struct.unpack_from("<H", raw, off + 16)[0] + 1
        xlen = struct.unpack_from("<H", raw, off + 10)[0]
        payload = raw[off + 12 + xlen: off + bsize - 8]
        comps.append(payload); sizes.append(struct.unpack_from("<I", raw, off + bsize - 4)[0]); want.append(zlib.decompress(payload, -15))
        off += bsize
    assert len(comps) > 70                                        # more than one wave of blocks
    rc, out, o = _gpu_inflate(gpu_lib, comps, sizes)
    assert rc == 0, gpu_lib.last_error()
    for k in range(len(comps)):
        assert out[o[k]:o[k] + sizes[k]].tobytes() == want[k], k
    bad = list(comps); b = bytearray(bad[40]); b[len(b) // 2] ^= 0x10; bad[40] = bytes(b)
    rc, out, o = _gpu_inflate(gpu_lib, bad, sizes)
    if rc == 0:
        assert out[o[40]:o[40] + sizes[40]].tobytes() != want[40]   # a flip that still decodes to ISIZE bytes is the CRC's to find
    else:
        assert "block 40" in gpu_lib.last_error()


@pytest.mark.gpu
def test_device_inflate_of_the_catalogue(gpu_lib, kernel_form, catalogue):
    """every stream of tests/deflate_streams.py in ONE call: the wave forms' scalar symbol loop (bit-by-bit codes, the deferred store of a short
    match, the hand-back of the bit position at a block boundary) exists only in the device build"""
    rc, out, off = _gpu_inflate(gpu_lib, [c.comp for c in catalogue], [len(c.out) for c in catalogue])
    assert rc == 0, gpu_lib.last_error()
    for c, o in zip(catalogue, off):
        got = out[o:o + len(c.out)].tobytes()
        if got != c.out:
            at = next(i for i in range(len(c.out)) if got[i] != c.out[i])
            assert False, "%s: first differing byte %d of %d" % (c.name, at, len(c.out))
    total = sum(len(c.out) for c in catalogue)
    assert (out[:100] == 0xAB).all() and (out[100 + total:] == 0xAB).all()


@pytest.mark.gpu
def test_device_inflate_batch_shapes(gpu_lib, kernel_form, catalogue):
    """calls of 1..5 and 65 blocks (four blocks per workgroup in the wave forms, 64 in the lane form: the i >= n tails of both), and blocks of
    ISIZE 0 first, in the middle and last among others"""
    small = [c for c in catalogue if 0 < len(c.out) <= 1500]
    empty = [c for c in catalogue if c.name in ("only_empty_fixed", "only_empty_stored")]
    assert len(small) >= 20 and len(empty) == 2
    batches = [[small[(7 * n + k) % len(small)] for k in range(n)] for n in (1, 2, 3, 4, 5, 65)]
    batches += [[empty[0], small[0], small[1], empty[1], small[2], empty[0], small[3], empty[1]], [empty[1], small[4], empty[0]], [small[5], empty[0], empty[1], small[6]]]
    for batch in batches:
        rc, out, off = _gpu_inflate(gpu_lib, [c.comp for c in batch], [len(c.out) for c in batch])
        assert rc == 0, (len(batch), gpu_lib.last_error())
        for k, (c, o) in enumerate(zip(batch, off)):
            assert out[o:o + len(c.out)].tobytes() == c.out, (len(batch), k, c.name)
        total = sum(len(c.out) for c in batch)
        assert (out[:100] == 0xAB).all() and (out[100 + total:] == 0xAB).all(), len(batch)


@pytest.mark.gpu
def test_device_inflate_names_the_invalid_block(gpu_lib, kernel_form, catalogue):
    """the structured invalid streams, one per call, as the middle block of three: the call fails and the message names block 1 and the
    error of the rule the stream breaks, the same as on the host (tests/deflate_streams.py: core_rc).  (What the
    neighbours' outputs hold after a failed call is undefined by the function's contract and not looked at.)"""
    by_name = {c.name: c for c in catalogue}
    before, after = by_name["one_distance_code"], by_name["fixed_11_literals"]
    for c in deflate_streams.invalid_catalogue():
        rc, _, _ = _gpu_inflate(gpu_lib, [before.comp, c.comp, after.comp], [len(before.out), c.isize, len(after.out)])
        assert rc != 0, c.name
        assert "block 1 (code %d)" % c.core_rc in gpu_lib.last_error(), (c.name, gpu_lib.last_error())     # that block, refused by the rule it breaks


@pytest.mark.gpu
def test_device_inflate_is_as_lenient_as_the_host_core(gpu_lib, kernel_form, catalogue):
    """the two leniencies of test_decoder_core_is_more_lenient_than_zlib_in_two_places on the kernels, whose wave forms have their own copy of
    the bit-by-bit decode: an incomplete literal/length code and bytes behind the final block decode, as middle blocks, to the bytes the
    builder's tokens give (zlib refuses the first).  The stream that uses an unassigned code of the incomplete code is one of
    test_device_inflate_names_the_invalid_block's."""
    by_name = {c.name: c for c in catalogue}
    before, after = by_name["one_distance_code"], by_name["fixed_11_literals"]
    for name, comp, want in deflate_streams.lenient_catalogue():
        batch = [(before.comp, before.out), (comp, want), (after.comp, after.out)]
        rc, out, off = _gpu_inflate(gpu_lib, [c for c, _ in batch], [len(w) for _, w in batch])
        assert rc == 0, (name, gpu_lib.last_error())
        for (_, w), o in zip(batch, off):
            assert out[o:o + len(w)].tobytes() == w, name
        total = sum(len(w) for _, w in batch)
        assert (out[:100] == 0xAB).all() and (out[100 + total:] == 0xAB).all(), name
