"""A synthetic targeted-panel input for uvc1-mi355x -R panel.bed [--merge-regions N]: one contig with reads over a stretch of `--kb` kb at
`--depth`x (duplex-UMI read names with --umi: the config-4 shape) and a BED file of `--lines` lines of 150-250 bp spread over the stretch.
    python scripts/make_panel.py OUT_DIR --kb 100 --depth 300 --lines 300
writes OUT_DIR/p.bam (+ .bai), p.fa (+ .fai), panel.bed.  tests/bamwriter.py writes the files (slow Python, not part of any timing)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import bamwriter                      # noqa: E402
from uvc_amd import synth             # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("out"); ap.add_argument("--kb", type=int, default=100); ap.add_argument("--depth", type=int, default=300)
ap.add_argument("--lines", type=int, default=300); ap.add_argument("--umi", action="store_true"); ap.add_argument("--seed", type=int, default=3)
a = ap.parse_args()
os.makedirs(a.out, exist_ok=True)
rng = np.random.default_rng(a.seed)
reads = synth.generate_region(seed=a.seed, region_len=a.kb * 1000, depth=a.depth, beg=50000, umi=a.umi, snv_every=300, somatic_every=900, indel_every=500)
umis = None
if a.umi:
    umis = ["".join("ACGT"[i] for i in rng.integers(0, 4, 6)) + "+" + "".join("ACGT"[i] for i in rng.integers(0, 4, 6)) for _ in range(int(reads["n_fams"]))]
recs = bamwriter.records_from_reads(reads, tid=0, umis=umis)
chrom_len = reads["end"] + 50000
seq = "".join("ACGT"[i] for i in rng.integers(0, 4, chrom_len))
seq = seq[:reads["beg"]] + reads["refseq"] + seq[reads["end"]:]
bamwriter.write_bam(os.path.join(a.out, "p.bam"), [("chrP", chrom_len)], recs)
bamwriter.write_fasta(os.path.join(a.out, "p.fa"), [("chrP", seq)])
pitch = (a.kb * 1000 - 600) // a.lines
assert pitch > 260, "too many lines for the stretch"
with open(os.path.join(a.out, "panel.bed"), "w") as f:
    for i in range(a.lines):
        b = reads["beg"] + 300 + i * pitch + int(rng.integers(0, pitch - 255))
        f.write("chrP\t%d\t%d\n" % (b, b + int(rng.integers(150, 251))))
print("%d reads, %d BED lines, BAM %.1f MB" % (len(recs), a.lines, os.path.getsize(os.path.join(a.out, "p.bam")) / 1e6))
