"""Pair mode of uvc1-mi355x (--normal-bam) and the in-memory tumor store of libuvcio, without a device: the options are listed, each side
resolves its parameters as its two-pass command line does (uvcTN.sh:27-50, 120-127), the refusals come before any file or device, and
the store answers every fetch as the file-backed reader does on the same lines."""
import random
import struct
import threading

import numpy as np

from test_cli_params_cpu import help_classes, run, write_bam
from uvc_amd import io as uio


def test_pair_options_are_listed_as_cli():
    classes = help_classes()
    for n in ("--normal-bam", "--tumor-output", "--tumor-params", "--normal-params"):
        assert classes.get(n) == "CLI", n


def params_of(args):
    r = run(args)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


def pair_blocks(args):
    lines = params_of(args)
    t = [l[len("tumor."):] for l in lines if l.startswith("tumor.")]
    n = [l[len("normal."):] for l in lines if l.startswith("normal.")]
    assert len(t) + len(n) == len(lines) and len(t) == len(n) > 100
    assert lines == ["tumor." + l for l in t] + ["normal." + l for l in n]   # the tumor block, then the normal block
    return t, n


def test_print_params_blocks_equal_the_two_pass_command_lines(tmp_path):
    tb, nb = write_bam(tmp_path, "tum", True, 35), write_bam(tmp_path, "nor", False, 24)   # Illumina-like tumor, IonTorrent-like normal
    bed = tmp_path / "T.bed"                                                                  # the tumor pass's region table of the same span
    bed.write_text("chrP\t0\t20000\n")
    shared = ["-t", "2", "--tile", "5000", "--fam-thres-dup1add", "3"]
    tside, nside = ["--fam-thres-highBQ-snv", "27"], ["--tn-syserr-norm-devqual", "-1.0"]
    t, n = pair_blocks([tb, "--normal-bam", nb, "--tumor-output", "t.vcf.gz", "--print-params"] + shared + ["--tumor-params"] + tside + ["--normal-params"] + nside)
    t2 = params_of([tb, "--tn-is-paired", "1", "--print-params"] + shared + tside)
    n2 = params_of([nb, "--tn-is-paired", "1", "--bed-in-fname", str(bed), "--tumor-vcf", "T.vcf.gz", "--print-params"] + shared + nside)
    assert t == t2 and n == n2
    td, nd = dict(l.split("=", 1) for l in t), dict(l.split("=", 1) for l in n)
    assert td["inferred_sequencing_platform"] != nd["inferred_sequencing_platform"]             # each side infers from its own BAM
    assert td["fam_thres_highBQ_snv"] == "27" and nd["fam_thres_highBQ_snv"] != "27"
    assert nd["tn_syserr_norm_devqual"] == "-1" and td["tn_syserr_norm_devqual"] != "-1"
    assert td["tn_is_paired"] == nd["tn_is_paired"] == "1"                                      # uvcTN.sh's --tn-is-paired 1 on both sides
    assert td["fam_thres_dup1add"] == nd["fam_thres_dup1add"] == "3" and nd["tumor_vcf_is_provided"] == "1"
    # the reference's own cuts: the normal side reads the tumor's regions back, as the two-pass flow reads the tumor's region table
    B = uio.Bam(tb)
    cols = B.fetch(0, 0, 20000)
    cuts = uio.plan_regions(cols["tid"], cols["pos"], cols["endpos"], cols["flag"], [20000], nthreads=2, mem_per_thread_mb=1)
    assert len(cuts) >= 2
    cut_bed = tmp_path / "cuts.bed"
    cut_bed.write_text("".join("chrP\t%d\t%d\n" % (c["beg"], c["end"]) for c in cuts))
    t, n = pair_blocks([tb, "--normal-bam", nb, "--tumor-output", "t.vcf.gz", "--print-params", "-t", "2", "--mem-per-thread", "1"])
    assert t == params_of([tb, "--tn-is-paired", "1", "--print-params", "-t", "2", "--mem-per-thread", "1"])
    assert n == params_of([nb, "--tn-is-paired", "1", "--bed-in-fname", str(cut_bed), "--tumor-vcf", "T.vcf.gz", "--print-params", "-t", "2", "--mem-per-thread", "1"])
    # a platform given on one side only
    t, n = pair_blocks([tb, "--normal-bam", nb, "--tumor-output", "t.vcf.gz", "--print-params", "--normal-params", "--sequencing-platform", "1"])
    assert n == params_of([nb, "--tn-is-paired", "1", "--bed-in-fname", str(bed), "--tumor-vcf", "T.vcf.gz", "--print-params", "--sequencing-platform", "1"])


BASE = ["/no/such.bam", "-f", "/no/such.fa", "-o", "/no/such/n.vcf.gz"]
PAIR = BASE + ["--normal-bam", "/no/such2.bam", "--tumor-output", "/no/such/t.vcf.gz"]


def test_pair_refusals_come_before_any_file_or_device():
    cases = [
        (PAIR + ["--tumor-vcf", "/no/such/t.vcf.gz"], "--tumor-vcf"),
        (PAIR + ["--bed-in-fname", "/no/such.bed"], "--bed-in-fname"),
        (PAIR + ["--bed-in-fname=/no/such.bed"], "--bed-in-fname"),
        (BASE + ["--normal-bam", "/no/such2.bam"], "--tumor-output"),
        (BASE + ["--normal-bam", "/no/such2.bam", "--tumor-output", "/no/such/n.vcf.gz"], "--tumor-output"),
        (BASE + ["--tumor-params", "--fam-thres-highBQ-snv", "27"], "--tumor-params"),
        (BASE + ["--normal-params", "--fam-thres-highBQ-snv", "27"], "--normal-params"),
        (PAIR + ["--tumor-params", "-t", "2"], "-t"),
        (PAIR + ["--normal-params", "--tile", "500"], "--tile"),
        (PAIR + ["--normal-params", "--bed-out-fname=/no/such.bed"], "--bed-out-fname"),
        (["/only-print-vcf-header/", "--normal-bam", "/no/such2.bam", "--tumor-output", "/no/such/t.vcf.gz"], "/only-print-vcf-header/"),
        (PAIR + ["--tumor-params", "--fam-thres-highBQ-snv", "x"], "--fam-thres-highBQ-snv"),
    ]
    for args, named in cases:
        for mode in ([], ["--print-params"]):
            r = run(mode + args)
            assert r.returncode == 2 and named in r.stderr, (args, r.stderr)
            assert "such" not in r.stderr and "HIP" not in r.stderr, r.stderr


FMT = "GT:VTI:BDPb:bDPf:bDPr:CDP1x:cDP1x:cVQ1:cPCQ1:CDP2x:cDP2x:cVQ2:cPCQ2:bNMQ:vHGQ:CDP1b:cDP1f:cDP1r:CDP2b"


def smp(vti, k):
    return "./1:%s:%d,%d:9,%d:8,%d:%d:100,%d:50,%d:60,%d:%d:10,%d:40,%d:45,%d:30,%d:%d:70,%d:20,%d:21,%d:5,%d" % (
        vti, 100 + k, 90 + k, 3 + k, 4 + k, 9000 + k, 300 + k, 31 + k, 32 + k, 800 + k, 30 + k, 41 + k, 42 + k, 17 + k, 55 + k, 60 + k, 6 + k, 7 + k, 1 + k)


def tumor_lines(rng, n):
    """Record lines of a tumor VCF in genome order: substitutions, InDels, MGVCF blocks, extra InDel candidates, several records per
    position, a symbolic allele the reader skips and a contig the BAM does not have."""
    out, pos = [], {"chrA": 1, "chrB": 1}
    for k in range(n):
        chrom = "chrA" if k < n * 2 // 3 else "chrB"
        pos[chrom] += int(rng.integers(0, 4))
        p = pos[chrom]
        kind = int(rng.integers(0, 7))
        if kind == 0: out.append("%s\t%d\t.\tC\tT\t50\tPASS\tANY_VAR\t%s\t%s" % (chrom, p, FMT, smp("1,3", k)))
        elif kind == 1: out.append("%s\t%d\t.\tGAC\tG\t50\tPASS\tANY_VAR\t%s:_C2XP\t%s:x" % (chrom, p, FMT, smp("6,8", k)))
        elif kind == 2: out.append("%s\t%d\t.\tG\tGTTT\t50\tPASS\tANY_VAR\t%s\t%s" % (chrom, p, FMT, smp("6,10", k)))
        elif kind == 3: out.append("%s\t%d\t.\tT\t<NON_REF>\t.\t.\tMGVCF_BLOCK\tGT:VTI:POS_VT_BDP_CDP_HomRefQ\t.:3,15:1000,2,.,5,5,5,30,.,2001" % (chrom, p))
        elif kind == 4: out.append("%s\t%d\t.\tT\t<ADDITIONAL_INDEL_CANDIDATE>\t.\t.\tADDITIONAL_INDEL_CANDIDATE;RU=A;RC=9\tGT:VTI:clipDP\t.:3,16:40,12" % (chrom, p))
        elif kind == 5: out.append("%s\t%d\t.\tA\t<DEL>\t50\tPASS\tANY_VAR\t%s\t%s" % (chrom, p, FMT, smp("1,2", k)))
        else: out.append("chrZ\t%d\t.\tA\tG\t50\tPASS\tANY_VAR\t%s\t%s" % (p, FMT, smp("0,2", k)))
    return out


def fetched(v, tid, a, b):
    keys, cols = v.fetch(tid, a, b)
    ras = v.last_ref_alt
    if keys is None:
        return []
    return [(bytes(k), c, r) for k, c, r in zip(keys, cols, ras)]


def chunks_with_edges(rng, lines):
    """The lines cut into tiles, each tile also holding the last lines of the one in front (the duplicated end point of two regions)."""
    cuts = sorted(set(int(x) for x in rng.integers(1, len(lines), 12)))
    out, at = [], 0
    for c in cuts + [len(lines)]:
        out.append(lines[max(0, at - int(rng.integers(0, 3))):c])
        at = c
    return out


def file_of(path, chunks):
    with open(path, "w") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tTUM\n")
        for c in chunks:
            f.write("".join(l + "\n" for l in c))
    return str(path)


def test_store_fetches_what_the_file_reader_fetches(tmp_path):
    rng = np.random.default_rng(3)
    names = ["chrA", "chrB"]
    for fmt in (True, False):
        chunks = chunks_with_edges(rng, tumor_lines(rng, 600))
        F = uio.TumorVcf(file_of(tmp_path / "t.vcf", chunks), names, is_tumor_format_retrieved=fmt)
        S = uio.TumorVcf.create("TUM", names, is_tumor_format_retrieved=fmt)
        assert S.sample == F.sample == "TUM" and S.n_records == 0
        order = list(range(len(chunks)))
        random.Random(5).shuffle(order)
        for i in order:
            S.add_lines("".join(l + "\n" for l in chunks[i]))
        assert S.n_records == F.n_records > 150
        hi = max(int(l.split("\t")[1]) for c in chunks for l in c) + 5
        for _ in range(300):
            tid = int(rng.integers(0, 2))
            a = int(rng.integers(-5, hi)); b = a + int(rng.integers(0, 80))
            assert fetched(S, tid, a, b) == fetched(F, tid, a, b), (tid, a, b)
        assert fetched(S, 0, 0, 10 ** 9) == fetched(F, 0, 0, 10 ** 9) and len(fetched(S, 1, 0, 10 ** 9)) > 50
        assert fetched(S, 2, 0, 10 ** 9) == [] and fetched(S, -1, 0, 10 ** 9) == []
        F.close(); S.close()


def test_store_adds_and_fetches_on_several_threads(tmp_path):
    """Adds in genome order from one thread, fetches from three others that check the records of ranges whose tiles are all in."""
    rng = np.random.default_rng(4)
    names = ["chrA", "chrB"]
    chunks = chunks_with_edges(rng, tumor_lines(rng, 1500))
    F = uio.TumorVcf(file_of(tmp_path / "t.vcf", chunks), names)
    S = uio.TumorVcf.create("TUM", names)
    hi = max(int(l.split("\t")[1]) for c in chunks for l in c) + 5
    added = [0]
    errors = []
    lock = threading.Lock()

    def adder():
        for c in chunks:
            S.add_lines("".join(l + "\n" for l in c))
            with lock:
                added[0] += 1

    def fetcher(seed):
        r = np.random.default_rng(seed)
        n_checked = 0
        while True:
            with lock:
                complete = added[0] == len(chunks)
            tid = int(r.integers(0, 2)); a = int(r.integers(0, hi)); b = a + int(r.integers(0, 60))
            got = fetched(S, tid, a, b)
            if complete:
                if got != fetched(F, tid, a, b):
                    errors.append((tid, a, b))
                n_checked += 1
                if n_checked >= 200:
                    return
            else:                                                 # while tiles come in: a consistent, ordered answer all the same
                keys = [struct.unpack("<ii", g[0][:8]) for g in got]
                if keys != sorted(keys) or any(not (a <= k[0] <= b) for k in keys):
                    errors.append(("order", tid, a, b))

    th = [threading.Thread(target=adder)] + [threading.Thread(target=fetcher, args=(s,)) for s in range(3)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors[:5]
    assert S.n_records == F.n_records
    F.close(); S.close()
