"""Divergence of a set of assemblies, estimated on the GPU the way Mash does it (`ntSynt -d auto`, bin/ntsynt_divergence).

Each genome is reduced to a bottom-s MinHash sketch: the s smallest distinct canonical ntHash values (h0) of its valid k-mers
(nts_minhash, csrc/nts_minhash.inc -- exact, not approximate).  For a pair, with U = bottom-s(A u B):

    j = |U n A n B| / |U|,    D = -ln(2j / (1 + j)) / k    (D = 1 when j = 0; at most 1)

which estimates the per-base substitution distance -ln(1 - p).  The hash is ntSynt's ntHash, not Mash's MurmurHash, so
distances are comparable with Mash's but not bit-identical.  The suggested `-d` is 100 x the largest pairwise D, rounded up to
0.001 (docs/design/04_7_divergence_estimate.md)."""
import math
from dataclasses import dataclass, field

import numpy as np

K_DEFAULT = 21          # Mash's k
S_DEFAULT = 10000       # ten times Mash's sketch size: the sweep costs the same


def sketch(genome, k=K_DEFAULT, s=S_DEFAULT):
    "bottom-s sketch of a resident genome (device.Genome): uint64, ascending, distinct"
    return genome.minhash(k, s)


def merge(a, b, s):
    "bottom-s of the union of two sketches: exact, so the sketches of a genome's record slices merge into the genome's sketch"
    return np.union1d(np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64))[:int(s)]


def distance_of_counts(shared, size, k):
    "Mash distance from shared = |bottom-s(A u B) n A n B| and size = |bottom-s(A u B)|"
    shared, size = int(shared), int(size)
    if size == 0 or shared == 0:
        return 1.0
    if shared == size:
        return 0.0
    j = shared / size
    return min(1.0, -math.log(2.0 * j / (1.0 + j)) / int(k))


def distance(a, b, k, s):
    "(Mash distance, shared hashes, |bottom-s(A u B)|) of two sketches"
    a = np.asarray(a, dtype=np.uint64)
    b = np.asarray(b, dtype=np.uint64)
    u = merge(a, b, s)
    shared = int(np.intersect1d(np.intersect1d(u, a, assume_unique=True), b, assume_unique=True).size)
    return distance_of_counts(shared, u.size, k), shared, int(u.size)


def suggested_divergence(d_max):
    "ntSynt's -d (percent) for the largest pairwise distance: 100 x d_max rounded UP to 0.001"
    return math.ceil(round(100.0 * d_max * 1000.0, 6)) / 1000.0


@dataclass
class Estimate:
    names: list                     # the genomes, in input order
    k: int
    s: int
    pairs: list = field(default_factory=list)   # (i, j, distance, shared hashes, sketch size), i < j, in input order
    divergence: float = 0.0         # suggested -d, percent
    largest: tuple = (0, 1)         # (i, j) of the pair with the largest distance

    def table(self):
        "TSV with a header, one line per unordered pair, then `# ntSynt -d <value>`"
        lines = ["genome_a\tgenome_b\tdistance\tshared_hashes\tsketch_size"]
        for i, j, d, shared, size in self.pairs:
            lines.append(f"{self.names[i]}\t{self.names[j]}\t{d:.6g}\t{shared}\t{size}")
        lines.append(f"# ntSynt -d {self.divergence}")
        return "\n".join(lines) + "\n"

    def summary(self):
        a, b = self.largest
        return (f"Estimated percent divergence: {self.divergence} (largest pair: {self.names[a]} vs {self.names[b]}; "
                f"k {self.k}, sketch {self.s})")


def from_sketches(names, sketches, k=K_DEFAULT, s=S_DEFAULT):
    "pairwise table and suggested -d of sketches already made"
    est = Estimate(names=list(names), k=int(k), s=int(s))
    d_max, largest = -1.0, (0, 1)
    for i in range(len(sketches)):
        for j in range(i + 1, len(sketches)):
            d, shared, size = distance(sketches[i], sketches[j], k, s)
            est.pairs.append((i, j, d, shared, size))
            if d > d_max:
                d_max, largest = d, (i, j)
    est.divergence = suggested_divergence(max(d_max, 0.0))
    est.largest = largest
    return est


def estimate(fastas, k=K_DEFAULT, s=S_DEFAULT, device=0, ctx=None):
    """Sketch every FASTA on the GPU, one genome resident at a time (read with the GPU parse, sketched, freed), and return the
    Estimate over all pairs.  At least two files."""
    if len(fastas) < 2:
        raise ValueError("a divergence estimate needs at least two genomes")
    from .device import Context
    from .fasta import read_fasta_device
    own = ctx is None
    ctx = ctx or Context(device)
    try:
        sketches = []
        for path in fastas:
            g, _ = read_fasta_device(ctx, path)
            try:
                sketches.append(sketch(g, k, s))
            finally:
                g.free()
    finally:
        if own:
            ctx.close()
    return from_sketches(fastas, sketches, k, s)
