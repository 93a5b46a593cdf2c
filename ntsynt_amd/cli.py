"""`ntSynt` command line of the HIP path: same flags, defaults, validation and messages as the
reference driver (bin/ntSynt:43-170), with the Snakemake hop replaced by an in-process GPU pipeline.

Differences a user can see: `-t` is accepted but unused (the GPU does the work), `-n/--dry-run` prints
the stage plan instead of Snakemake's, `--benchmark` writes {prefix}.stage_times.tsv, `-f/--force` is
accepted (every run recomputes everything)."""
import argparse
import os
import sys

NTSYNT_VERSION = "ntSynt v1.0.4 (ntsynt_amd / MI355X)"

NTSYNT_BANNER = "ntSynt on MI355X -- minimizer-graph macrosynteny, sketch / Bloom filter / graph stage in HBM"


def read_fasta_files(filename):
    "one FASTA path per line (bin/ntSynt:25-31)"
    with open(filename, "r", encoding="utf-8") as fin:
        return [line.strip() for line in fin]


def divergence_value(text):
    "-d: a percentage, or `auto` (estimated on the GPU from the genomes: ntsynt_amd/divergence.py)"
    if text == "auto":
        return text
    return float(text)


divergence_value.__name__ = "float"        # argparse's message for a bad value stays "invalid float value: ..."


def build_parser():
    epilog = "\n".join([
        "Parameters derived from -d unless given explicitly (the reference's table, bin/ntSynt:89-99):",
        "  -d below 1      block_size 500    indel 10000    merge 10000     w_rounds 100 10",
        "  -d 1 to 10      block_size 1000   indel 50000    merge 100000    w_rounds 250 100",
        "  -d above 10     block_size 10000  indel 100000   merge 1000000   w_rounds 500 250",
    ])
    p = argparse.ArgumentParser(prog="ntSynt", description="Macrosynteny blocks of two or more genome assemblies from a minimizer graph "
                                "(ntSynt's method and command line; all sequence-scale work on the GPU)",
                                formatter_class=argparse.RawTextHelpFormatter, epilog=epilog)
    p.add_argument("fastas", help="genome assemblies (FASTA, plain or .gz), two or more", nargs="*")
    p.add_argument("--fastas_list", help="text file naming the assemblies, one path per line (instead of positional arguments)",
                   required=False, type=str)
    p.add_argument("-d", "--divergence", help="upper estimate of the sequence divergence between the assemblies, in percent (-d 1 = 1%%);\n"
                   "selects --indel, --merge, --w_rounds and --block_size (table below);\n"
                   "`auto`: estimated from the assemblies on the GPU (Mash distance of MinHash sketches, k 21, sketch 10000)",
                   required=True, type=divergence_value)
    p.add_argument("-p", "--prefix", help="prefix of the output files [ntSynt.k<k>.w<w>]", required=False)
    p.add_argument("-k", help="k-mer size of the minimizers [24]", type=int, required=False, default=24)
    p.add_argument("-w", help="window size of the minimizers [1000]", type=int, required=False, default=1000)
    p.add_argument("-t", help="threads [12]: accepted for compatibility with the reference, the GPU path does not use it", type=int, default=12)
    p.add_argument("--fpr", help="false positive rate the common Bloom filter is sized for [0.025]", default=0.025, type=float)
    p.add_argument("-b", "--block_size", help="shortest synteny block reported (bp)", type=int, required=False)
    p.add_argument("--merge", help="collinear blocks closer than this are merged (bp, or a multiple of the window size such as 3w)", type=str)
    p.add_argument("--w_rounds", help="window sizes of the refinement rounds, decreasing", nargs="+", type=int)
    p.add_argument("--indel", help="largest difference between assemblies in the distance of neighbouring minimizers before a block is split (bp)",
                   type=int)
    p.add_argument("--no-common", help=argparse.SUPPRESS, action="store_true")
    p.add_argument("--no-simplify-graph", help=argparse.SUPPRESS, action="store_true")
    p.add_argument("-n", "--dry-run", help="list the stages that would run, then stop", action="store_true")
    p.add_argument("--benchmark", help="write the wall-clock time of every stage to <prefix>.stage_times.tsv", action="store_true")
    p.add_argument("-f", "--force", help="accepted for compatibility (every run recomputes everything)", action="store_true")
    p.add_argument("--dev", help="developer mode: verbose log, overlap self-check of the final blocks", action="store_true")
    p.add_argument("--repeat", help=argparse.SUPPRESS, action="store_true")   # the Snakefile's experimental config "repeat": <prefix>.repeat.bf + indexlr -r
    p.add_argument("--interarrivals", help=argparse.SUPPRESS, action="store_true")   # ntsynt_run.py --interarrivals: <prefix>.interarrivals.tsv
    p.add_argument("--assess", help="after the run, write <prefix>.block_stats.tsv (number of blocks, coverage, mean / median length, NG50, N50)\n"
                   "and <prefix>.block_divergence.tsv (Mash distance of every block per pair of its genomes), from the genomes still on the GPU",
                   action="store_true")
    p.add_argument("--assess-k", help="k-mer size of the per-block sketches [21]", type=int, default=21)
    p.add_argument("--assess-s", help="size of the per-block sketches [1000]", type=int, default=1000)
    p.add_argument("--block-identity", help="after the run, write <prefix>.block_identity.tsv: per block and pair of its genomes the exact edit distance\n"
                   "of the stretches between consecutive anchors (sampled k-mers either genome has once), how much of the block they cover\n"
                   "and why the rest was not aligned, from the genomes still on the GPU", action="store_true")
    p.add_argument("--block-variants", help="after the run, write <prefix>.block_variants.tsv: the edits behind the `edits` of --block-identity, as snv /\n"
                   "ins / del events in both genomes' coordinates; works with or without --block-identity and takes the --identity-* parameters",
                   action="store_true")
    p.add_argument("--block-wide-variants", help="after the run, write <prefix>.block_wide_variants.tsv: the complete list of edits behind the `edits` of\n"
                   "--block-identity --identity-max-edits E, the large insertions and deletions of the stretches the band leaves out included;\n"
                   "needs --identity-max-edits E > 0, works with or without --block-identity", action="store_true")
    p.add_argument("--identity-k", help="k-mer size of the anchors [21]", type=int, default=21)
    p.add_argument("--identity-rate", help="sample one in this many k-mers as anchor candidates [16]", type=int, default=16)
    p.add_argument("--identity-band", help="half-width of the alignment band, 1..31 [31]", type=int, default=31)
    p.add_argument("--identity-max-len", help="longest stretch between two anchors that is aligned, 1..65535 [4096]", type=int, default=4096)
    p.add_argument("--identity-max-edits", help="with --block-identity or --block-wide-variants (which needs it): also align the stretches the band\n"
                   "leaves out (indels of 32 bases or more), up to this many edits: 0 = off, else 2 * --identity-band + 1 .. 1023;\n"
                   "not with --block-variants [0]", type=int, default=0)
    p.add_argument("--block-ends", help="after the run, write <prefix>.block_ends.tsv: per block and pair of its genomes the base-exact breakpoints --\n"
                   "how far the alignment continues in front of the first and behind the last aligned stretch of --block-identity, past the\n"
                   "block's own ends, and why it stops; works with or without --block-identity and takes the --identity-* parameters",
                   action="store_true")
    p.add_argument("--block-end-variants", help="with --block-ends (which it needs), write <prefix>.block_end_variants.tsv: the edits behind left_edits\n"
                   "and right_edits of --block-ends, as snv / ins / del events in both genomes' coordinates, flank by flank",
                   action="store_true")
    p.add_argument("--block-paf", help="after the run, write <prefix>.block_alignments.paf: one PAF record with a cg:Z: CIGAR (= X I D) per aligned\n"
                   "chain of every block and pair of its genomes; takes the --identity-* parameters (with --identity-max-edits E the stretches\n"
                   "beyond the band join the chains) and, with --block-ends, the --ends-* parameters (the flanks are attached); works with or\n"
                   "without the other block switches", action="store_true")
    p.add_argument("--paf-cs", help="with --block-paf (which it needs), every record also carries the cs:Z: tag (short form: :n, *tq, -bases, +bases)\n"
                   "behind cg:Z:, as paftools.js call and dot-plot viewers read it; both tag texts are then made on the GPU", action="store_true")
    p.add_argument("--block-chain", help="after the run, write <prefix>.block_alignments.chain: one UCSC liftover chain per block and pair of its\n"
                   "genomes (target = the pair's first genome), the chains of --block-paf joined per pair with the stretches between them as\n"
                   "dt dq gaps, for liftOver, CrossMap and genome browsers; takes the parameters of --block-paf; works with or without it",
                   action="store_true")
    p.add_argument("--block-maf", help="after the run, write <prefix>.block_alignments.maf: one pairwise MAF block per record of --block-paf with the\n"
                   "aligned sequences themselves (target = the pair's first genome, gaps as -, upper case, no soft-masking), both rows of every\n"
                   "chain made on the GPU, for conservation and phylogeny tools, MAF converters and browsers; takes the parameters of\n"
                   "--block-paf; works with or without it", action="store_true")
    p.add_argument("--block-maf-multi", help="after the run, write <prefix>.block_alignments.multi.maf: one reference-anchored multiple alignment per synteny\n"
                   "block -- all its genomes in shared columns, anchored on the block's first line, cut into sub-blocks where the covering genomes\n"
                   "change --, the gap columns and the rows made on the GPU; takes the parameters of --block-paf; works with or without the other\n"
                   "block switches; a pass of its own", action="store_true")
    p.add_argument("--block-conservation", help="after the run, write <prefix>.block_conservation.bed and <prefix>.block_conservation.tsv: per synteny\n"
                   "block the runs of bases of its first line with one (aligned, match, mismatch, gap) over the star alignment of\n"
                   "--block-maf-multi -- how many of the other genomes cover a base, and in how many it is identical --, made on the GPU, and\n"
                   "per block the covered, core and conserved bases with their histograms; takes the parameters of --block-paf; works with or\n"
                   "without the other block switches; a pass of its own", action="store_true")
    p.add_argument("--block-variant-sites", help="after the run, write <prefix>.block_variant_sites.tsv: per synteny block the positions of its\n"
                   "first line at which the other genomes differ over the star alignment of --block-maf-multi, one line per allele (snv / del /\n"
                   "ins with its letters), the genomes that share it and one genotype character per row, the bases and the allele table made on\n"
                   "the GPU; takes the parameters of --block-paf; works with or without the other block switches; a pass of its own",
                   action="store_true")
    p.add_argument("--block-consensus", help="after the run, write <prefix>.block_profile.tsv and <prefix>.block_consensus.fa: per synteny block one line\n"
                   "per variable column of the star alignment of --block-maf-multi -- reference bases and insertion columns alike -- with how\n"
                   "many genomes hold A, C, G, T, N or a gap there, the reference row counted in, and the plurality call, the tallies made on\n"
                   "the GPU; and per block its first line's bases with the calls applied; takes the parameters of --block-paf; works with or\n"
                   "without the other block switches; a pass of its own", action="store_true")
    p.add_argument("--block-lift", metavar="BED", help="after the run, write <prefix>.block_lift.tsv: the intervals of this BED file, which lie on the\n"
                   "genome --lift-genome names, mapped through the alignments of --block-paf into the other genomes, one line per interval\n"
                   "and aligned chain it overlaps; takes the parameters of --block-paf; works with or without the other block switches")
    p.add_argument("--lift-genome", metavar="NAME", help="with --block-lift or --lift-windows: the genome the intervals lie on, a FASTA base name as in\n"
                   "column 2 of the block table")
    p.add_argument("--lift-identity", help="with --block-lift BED (which it needs), write <prefix>.block_lift_identity.tsv: the lines of\n"
                   "<prefix>.block_lift.tsv with, per lifted interval, its matches, mismatches, the bases either genome lacks, the runs of such\n"
                   "bases and the identity", action="store_true")
    p.add_argument("--lift-windows", metavar="W", help="with --lift-genome NAME (which it needs), write <prefix>.block_windows.tsv: the same columns for\n"
                   "windows of W bases over every record of NAME -- identity along the genome; works with or without --block-lift", type=int)
    p.add_argument("--lift-join", help="with --block-lift BED and/or --lift-windows W (it needs one of them), write <prefix>.block_lift_joined.tsv\n"
                   "and/or <prefix>.block_windows_joined.tsv: one line per interval and PAIR of block lines, the span joined across the pair's\n"
                   "chains, the counts over all of it and the bases of the stretches between the chains that no alignment covers", action="store_true")
    p.add_argument("--ends-max-len", help="longest flank that is extended, 1..65535 [4096]", type=int, default=4096)
    p.add_argument("--ends-max-edits", help="most edits within one flank, 1..1023 [255]", type=int, default=255)
    p.add_argument("--ends-penalty", help="what an edit costs the extension's score, against 2 for a matching pair of bases, 3..255 [6]", type=int,
                   default=6)
    p.add_argument("--gaps", help="after the run, write <prefix>.gaps.tsv (every stretch of every genome outside the blocks: its N bases and the\n"
                   "share of its k-mers that every genome has, from the common Bloom filter still on the GPU) and <prefix>.gap_summary.tsv",
                   action="store_true")
    p.add_argument("--gap-links", help="with --gaps (which it implies), write <prefix>.gap_links.tsv: the pairs of gaps of different genomes that\n"
                   "share sampled k-mers of the common Bloom filter, with the orientation of the shared stretch and whether both gaps lie\n"
                   "between the same two blocks", action="store_true")
    p.add_argument("--gap-block-links", help="with --gap-links (which it implies, and whose rate and minimum it shares), write <prefix>.gap_block_links.tsv:\n"
                   "where each gap's sampled k-mers lie inside the blocks of every genome, its own included (a second copy, a moved segment)",
                   action="store_true")
    p.add_argument("--gap-copies", help="with --gaps (which it implies), write <prefix>.gap_copies.tsv: how often each genome holds each gap's sampled\n"
                   "k-mers, genome-wide, and whether the gap is unique everywhere, a repeat of its own genome or neither (shares --gap-links-rate)",
                   action="store_true")
    p.add_argument("--gap-copy-sites", help="with --gap-copies (which it implies, and whose rate it shares), write <prefix>.gap_copy_sites.tsv: where each\n"
                   "genome, the gap's own included, holds each gap's sampled k-mers close together -- the other copies of a repeat gap\n"
                   "(shares --gap-links-min)", action="store_true")
    p.add_argument("--gap-periods", help="with --gaps (which it implies), write <prefix>.gap_periods.tsv: per gap, the period, the copy count and the extent\n"
                   "of a tandem array in it, from an unfiltered sample of its k-mers (shares --gap-links-rate and --gap-links-min)",
                   action="store_true")
    p.add_argument("--gap-families", help="with --gap-periods (which it implies), write <prefix>.gap_families.tsv and <prefix>.gap_family_sites.tsv: which\n"
                   "tandem arrays share the hashes that carry their period, and where each genome holds each such family, inside the gaps\n"
                   "and inside the blocks (shares --gap-links-rate, --gap-links-min and --gap-sites-step)", action="store_true")
    p.add_argument("--gap-sites-cap", help="use a k-mer against a genome that holds it at most this many times [16]", type=int, default=16)
    p.add_argument("--gap-sites-step", help="two hits of a site lie at most this many bases apart [1000]", type=int, default=1000)
    p.add_argument("--gap-links-rate", help="sample one in this many of the gap k-mers the filter holds [16]", type=int, default=16)
    p.add_argument("--gap-links-min", help="anchors (sampled k-mers in common, unique in every genome) a link needs [4]", type=int, default=4)
    p.add_argument("--device", help="GPU index [0]", type=int, default=0)
    # switches for the two btllib details this implementation recalls rather than reads
    p.add_argument("--bf-rounding", help=argparse.SUPPRESS, choices=["up", "down", "none"], default="up")
    p.add_argument("--bf-signature", help=argparse.SUPPRESS, default=None)
    p.add_argument("-v", "--version", action="version", version=NTSYNT_VERSION)
    return p


def resolve(parser, args):
    "divergence -> defaults and input validation (bin/ntSynt:86-120,141-143)"
    if not args.prefix:
        args.prefix = f"ntSynt.k{args.k}.w{args.w}"
    if args.divergence < 1:
        args.indel, args.merge, args.w_rounds, args.block_size = \
            args.indel or 10000, args.merge or 10000, args.w_rounds or [100, 10], args.block_size or 500
    elif 1 <= args.divergence <= 10:
        args.indel, args.merge, args.w_rounds, args.block_size = \
            args.indel or 50000, args.merge or 100000, args.w_rounds or [250, 100], args.block_size or 1000
    elif 10 < args.divergence <= 100:
        args.indel, args.merge, args.w_rounds, args.block_size = \
            args.indel or 100000, args.merge or 1000000, args.w_rounds or [500, 250], args.block_size or 10000
    else:
        parser.error("--divergence must be a value between 0 and 100")
    for w in args.w_rounds:
        if w > args.w:
            parser.error("All values specified for --w_rounds must be smaller than -w")
    return input_fastas(parser, args)


def input_fastas(parser, args):
    "the assemblies named on the command line, after the checks that do not depend on the divergence (bin/ntSynt:114-120)"
    if not args.fastas and not args.fastas_list:
        parser.error("Please supply the input genome fasta files as positional arguments, "
                     "or specify a file listing the files (one fasta per line) with --fastas_list")
    if args.fastas and args.fastas_list:
        parser.error("Please supply the input genome fasta files as positional arguments, "
                     "or specify a single file (one fasta per line) with --fastas_list, NOT both.")
    fastas = read_fasta_files(args.fastas_list) if args.fastas_list else args.fastas
    if len(fastas) < 2:
        parser.error("Must supply at least two reference genomes to compare")
    return fastas


def estimate_divergence(parser, args, say):
    """-d auto: every check that does not depend on the divergence first, then the estimate over all genomes (under torchrun every
    rank makes the same exact estimate on its own GPU), then args.divergence = the printed value, as if it had been given"""
    fastas = input_fastas(parser, args)
    for fasta in fastas:
        if not os.path.isfile(fasta):
            raise FileNotFoundError(f"Input file {fasta} not found.")
    device = args.device
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:              # the GPU this rank will run on (main, below)
        device = int(os.environ.get("LOCAL_RANK", "0"))
        if os.environ.get("NTS_DIST_BACKEND", "nccl") != "nccl":
            import torch
            device %= max(torch.cuda.device_count(), 1)
    from . import divergence
    est = divergence.estimate(fastas, k=divergence.K_DEFAULT, s=divergence.S_DEFAULT, device=device)
    say(est.summary(), flush=True)
    args.divergence = float(str(est.divergence))


def check_reports(parser, args):
    "the switches of the reports behind the run (--assess, --gaps, --gap-links, --gap-block-links, --gap-copies, --gap-copy-sites, --gap-periods, --gap-families): what each implies and where each is refused"
    if args.assess:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            parser.error("--assess works from the genomes resident on one GPU: run it on one rank, or assess the finished run with "
                         "ntsynt_block_stats --tsv <prefix>.synteny_blocks.tsv --fai ... --fastas ...")
        if args.assess_k < 1 or args.assess_s < 1:
            parser.error("--assess-k and --assess-s must be positive")
    if args.block_variants:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            parser.error("--block-variants works from the genomes resident on one GPU: run it on one rank, or assess the finished run with "
                         "ntsynt_block_stats --tsv <prefix>.synteny_blocks.tsv --fai ... --fastas ... --variants-out <prefix>.block_variants.tsv")
    if args.block_wide_variants:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            parser.error("--block-wide-variants works from the genomes resident on one GPU: run it on one rank, or assess the finished run with "
                         "ntsynt_block_stats --tsv <prefix>.synteny_blocks.tsv --fai ... --fastas ... --identity-max-edits E "
                         "--wide-variants-out <prefix>.block_wide_variants.tsv")
    if args.block_identity or args.block_variants or args.block_wide_variants:
        if args.block_identity and int(os.environ.get("WORLD_SIZE", "1")) > 1:
            parser.error("--block-identity works from the genomes resident on one GPU: run it on one rank, or assess the finished run with "
                         "ntsynt_block_stats --tsv <prefix>.synteny_blocks.tsv --fai ... --fastas ... --identity-out <prefix>.block_identity.tsv")
        from .assess import WIDE_NOT_WITH_VARIANTS, WIDE_VARIANTS_NEED_E, check_identity_parameters
        message = check_identity_parameters(args.identity_k, args.identity_rate, args.identity_band, args.identity_max_len, args.identity_max_edits)
        if message:
            parser.error(message)
        if args.identity_max_edits and args.block_variants:
            parser.error(WIDE_NOT_WITH_VARIANTS)
        if args.block_wide_variants and not args.identity_max_edits:
            parser.error("--block-wide-variants: " + WIDE_VARIANTS_NEED_E)
    if args.block_end_variants:
        if not args.block_ends:
            from .assess import END_VARIANTS_NEED_ENDS
            parser.error("--block-end-variants: " + END_VARIANTS_NEED_ENDS)
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            parser.error("--block-end-variants works from the genomes resident on one GPU: run it on one rank, or assess the finished run with "
                         "ntsynt_block_stats --tsv <prefix>.synteny_blocks.tsv --fai ... --fastas ... --ends-out <prefix>.block_ends.tsv "
                         "--end-variants-out <prefix>.block_end_variants.tsv")
    if args.paf_cs:
        if not args.block_paf:
            parser.error("--paf-cs adds the cs:Z: tag to the records of --block-paf: it needs that switch")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            parser.error("--paf-cs works from the genomes resident on one GPU: run it on one rank, or assess the finished run with "
                         "ntsynt_block_stats --tsv <prefix>.synteny_blocks.tsv --fai ... --fastas ... --paf-out <prefix>.block_alignments.paf --paf-cs")
    if args.block_paf:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            parser.error("--block-paf works from the genomes resident on one GPU: run it on one rank, or assess the finished run with "
                         "ntsynt_block_stats --tsv <prefix>.synteny_blocks.tsv --fai ... --fastas ... --paf-out <prefix>.block_alignments.paf")
        from .assess import check_identity_parameters
        message = check_identity_parameters(args.identity_k, args.identity_rate, args.identity_band, args.identity_max_len, args.identity_max_edits)
        if message:
            parser.error(message)
    if args.block_chain:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            parser.error("--block-chain works from the genomes resident on one GPU: run it on one rank, or assess the finished run with "
                         "ntsynt_block_stats --tsv <prefix>.synteny_blocks.tsv --fai ... --fastas ... --chain-out <prefix>.block_alignments.chain")
        from .assess import check_identity_parameters
        message = check_identity_parameters(args.identity_k, args.identity_rate, args.identity_band, args.identity_max_len, args.identity_max_edits)
        if message:
            parser.error(message)
    if args.block_maf:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            parser.error("--block-maf works from the genomes resident on one GPU: run it on one rank, or assess the finished run with "
                         "ntsynt_block_stats --tsv <prefix>.synteny_blocks.tsv --fai ... --fastas ... --maf-out <prefix>.block_alignments.maf")
        from .assess import check_identity_parameters
        message = check_identity_parameters(args.identity_k, args.identity_rate, args.identity_band, args.identity_max_len, args.identity_max_edits)
        if message:
            parser.error(message)
    if args.block_maf_multi:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            parser.error("--block-maf-multi works from the genomes resident on one GPU: run it on one rank, or assess the finished run with "
                         "ntsynt_block_stats --tsv <prefix>.synteny_blocks.tsv --fai ... --fastas ... --multi-maf-out <prefix>.block_alignments.multi.maf")
        from .assess import check_identity_parameters
        message = check_identity_parameters(args.identity_k, args.identity_rate, args.identity_band, args.identity_max_len, args.identity_max_edits)
        if message:
            parser.error(message)
    if args.block_conservation:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            parser.error("--block-conservation works from the genomes resident on one GPU: run it on one rank, or assess the finished run with "
                         "ntsynt_block_stats --tsv <prefix>.synteny_blocks.tsv --fai ... --fastas ... --conservation-out <prefix>.block_conservation.bed "
                         "--conservation-stats-out <prefix>.block_conservation.tsv")
        from .assess import check_identity_parameters
        message = check_identity_parameters(args.identity_k, args.identity_rate, args.identity_band, args.identity_max_len, args.identity_max_edits)
        if message:
            parser.error(message)
    if args.block_variant_sites:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            parser.error("--block-variant-sites works from the genomes resident on one GPU: run it on one rank, or assess the finished run with "
                         "ntsynt_block_stats --tsv <prefix>.synteny_blocks.tsv --fai ... --fastas ... --variant-sites-out <prefix>.block_variant_sites.tsv")
        from .assess import check_identity_parameters
        message = check_identity_parameters(args.identity_k, args.identity_rate, args.identity_band, args.identity_max_len, args.identity_max_edits)
        if message:
            parser.error(message)
    if args.block_consensus:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            parser.error("--block-consensus works from the genomes resident on one GPU: run it on one rank, or assess the finished run with "
                         "ntsynt_block_stats --tsv <prefix>.synteny_blocks.tsv --fai ... --fastas ... --profile-out <prefix>.block_profile.tsv "
                         "--consensus-out <prefix>.block_consensus.fa")
        from .assess import check_identity_parameters
        message = check_identity_parameters(args.identity_k, args.identity_rate, args.identity_band, args.identity_max_len, args.identity_max_edits)
        if message:
            parser.error(message)
    if args.lift_genome and not args.block_lift and args.lift_windows is None:
        parser.error("--lift-genome names the genome of the intervals of --block-lift BED")
    if args.lift_identity:
        if not args.block_lift:
            parser.error("--lift-identity counts the alignment columns of the intervals of --block-lift BED: it needs that switch")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            parser.error("--lift-identity works from the genomes resident on one GPU: run it on one rank, or lift through the finished run with "
                         "ntsynt_block_stats --tsv <prefix>.synteny_blocks.tsv --fai ... --fastas ... --lift-bed BED --lift-genome NAME "
                         "--lift-identity-out <prefix>.block_lift_identity.tsv")
    if args.lift_join:
        if not args.block_lift and args.lift_windows is None:
            parser.error("--lift-join joins the lines of --block-lift BED and/or --lift-windows W per pair of block lines: it needs one of them")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            parser.error("--lift-join works from the genomes resident on one GPU: run it on one rank, or join through the finished run with "
                         "ntsynt_block_stats --tsv <prefix>.synteny_blocks.tsv --fai ... --fastas ... --lift-genome NAME --lift-bed BED "
                         "--lift-joined-out <prefix>.block_lift_joined.tsv [--lift-windows W --lift-windows-joined-out "
                         "<prefix>.block_windows_joined.tsv]")
    if args.lift_windows is not None:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            parser.error("--lift-windows works from the genomes resident on one GPU: run it on one rank, or count through the finished run with "
                         "ntsynt_block_stats --tsv <prefix>.synteny_blocks.tsv --fai ... --fastas ... --lift-genome NAME --lift-windows W "
                         "--lift-windows-out <prefix>.block_windows.tsv")
        if not args.lift_genome:
            parser.error("--lift-windows W needs --lift-genome NAME: the genome the windows lie on (a FASTA base name)")
        if args.lift_windows < 1:
            parser.error("--lift-windows W: a window has at least one base")
        names = [os.path.basename(path) for path in input_fastas(parser, args)]
        if args.lift_genome not in names:
            parser.error(f"--lift-genome {args.lift_genome} is not among the genomes {names}")
        from .assess import check_identity_parameters
        message = check_identity_parameters(args.identity_k, args.identity_rate, args.identity_band, args.identity_max_len, args.identity_max_edits)
        if message:
            parser.error(message)
    if args.block_lift:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            parser.error("--block-lift works from the genomes resident on one GPU: run it on one rank, or lift through the finished run with "
                         "ntsynt_block_stats --tsv <prefix>.synteny_blocks.tsv --fai ... --fastas ... --lift-bed BED --lift-genome NAME "
                         "--lift-out <prefix>.block_lift.tsv")
        if not args.lift_genome:
            parser.error("--block-lift BED needs --lift-genome NAME: the genome the intervals lie on (a FASTA base name)")
        names = [os.path.basename(path) for path in input_fastas(parser, args)]
        if args.lift_genome not in names:
            parser.error(f"--lift-genome {args.lift_genome} is not among the genomes {names}")
        from .assess import check_identity_parameters
        message = check_identity_parameters(args.identity_k, args.identity_rate, args.identity_band, args.identity_max_len, args.identity_max_edits)
        if message:
            parser.error(message)
    if args.block_ends:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            parser.error("--block-ends works from the genomes resident on one GPU: run it on one rank, or assess the finished run with "
                         "ntsynt_block_stats --tsv <prefix>.synteny_blocks.tsv --fai ... --fastas ... --ends-out <prefix>.block_ends.tsv")
        from .assess import check_ends_parameters, check_identity_parameters
        message = check_identity_parameters(args.identity_k, args.identity_rate, args.identity_band, args.identity_max_len, args.identity_max_edits) or \
            check_ends_parameters(args.ends_max_len, args.ends_max_edits, args.ends_penalty)
        if message:
            parser.error(message)
    if args.gap_block_links:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            parser.error("--gap-block-links works from the genomes resident on one GPU: run it on one rank, or report on the finished run with "
                         "ntsynt_gaps --tsv <prefix>.synteny_blocks.tsv --fastas ... --common <prefix>.common.bf "
                         "--block-links-out <prefix>.gap_block_links.tsv")
        if args.no_common:
            parser.error("--gap-block-links reads the common Bloom filter: not with --no-common")
        args.gap_links = True
    if args.gap_links:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            parser.error("--gap-links works from the genomes resident on one GPU: run it on one rank, or report on the finished run with "
                         "ntsynt_gaps --tsv <prefix>.synteny_blocks.tsv --fastas ... --common <prefix>.common.bf --links-out <prefix>.gap_links.tsv")
        if args.no_common:
            parser.error("--gap-links reads the common Bloom filter: not with --no-common")
        if args.gap_links_rate < 1 or args.gap_links_min < 1:
            parser.error("--gap-links-rate and --gap-links-min must be positive")
        args.gaps = True
    if args.gap_copy_sites:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            parser.error("--gap-copy-sites works from the genomes resident on one GPU: run it on one rank, or report on the finished run with "
                         "ntsynt_gaps --tsv <prefix>.synteny_blocks.tsv --fastas ... --common <prefix>.common.bf "
                         "--copy-sites-out <prefix>.gap_copy_sites.tsv")
        if args.no_common:
            parser.error("--gap-copy-sites reads the common Bloom filter: not with --no-common")
        if args.gap_links_min < 1 or not 1 <= args.gap_sites_cap <= 0xFFFFFFFF or not 0 <= args.gap_sites_step <= 0xFFFFFFFF:
            parser.error("--gap-links-min and --gap-sites-cap must be positive, --gap-sites-step not negative")
        args.gap_copies = True
    if args.gap_copies:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            parser.error("--gap-copies works from the genomes resident on one GPU: run it on one rank, or report on the finished run with "
                         "ntsynt_gaps --tsv <prefix>.synteny_blocks.tsv --fastas ... --common <prefix>.common.bf --copies-out <prefix>.gap_copies.tsv")
        if args.no_common:
            parser.error("--gap-copies reads the common Bloom filter: not with --no-common")
        if args.gap_links_rate < 1:
            parser.error("--gap-links-rate must be positive")
        args.gaps = True
    if args.gap_families:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            parser.error("--gap-families works from the genomes resident on one GPU: run it on one rank, or report on the finished run with "
                         "ntsynt_gaps --tsv <prefix>.synteny_blocks.tsv --fastas ... --common <prefix>.common.bf --families-out <prefix>.gap_families.tsv "
                         "--family-sites-out <prefix>.gap_family_sites.tsv")
        if args.no_common:
            parser.error("--gap-families reads the common Bloom filter: not with --no-common")
        if args.gap_links_rate < 1 or args.gap_links_min < 1:
            parser.error("--gap-links-rate and --gap-links-min must be positive")
        if args.gap_sites_step < 0 or args.gap_sites_step > 0xFFFFFFFF:
            parser.error("--gap-sites-step must not be negative (a 32-bit value)")
        args.gap_periods = True
    if args.gap_periods:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            parser.error("--gap-periods works from the genomes resident on one GPU: run it on one rank, or report on the finished run with "
                         "ntsynt_gaps --tsv <prefix>.synteny_blocks.tsv --fastas ... --common <prefix>.common.bf --periods-out <prefix>.gap_periods.tsv")
        if args.no_common:
            parser.error("--gap-periods reads the common Bloom filter: not with --no-common")
        if args.gap_links_rate < 1 or args.gap_links_min < 1:
            parser.error("--gap-links-rate and --gap-links-min must be positive")
        args.gaps = True
    if args.gaps:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            parser.error("--gaps works from the genomes resident on one GPU: run it on one rank, or report on the finished run with "
                         "ntsynt_gaps --tsv <prefix>.synteny_blocks.tsv --fastas ... --common <prefix>.common.bf")
        if args.no_common:
            parser.error("--gaps reads the common Bloom filter: not with --no-common")


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    rank0 = int(os.environ.get("RANK", "0")) == 0                # under torchrun every rank runs this; one of them talks
    say = print if rank0 else (lambda *a, **k: None)
    check_reports(parser, args)
    if args.divergence == "auto":
        estimate_divergence(parser, args, say)
    fastas = resolve(parser, args)
    say(NTSYNT_BANNER)
    say("\n".join(["Running ntSynt...",
                     f"Specified percent divergence: {args.divergence}",
                     "Parameter settings:",
                     f"\tfastas {fastas}",
                     f"\t--divergence {args.divergence}",
                     f"\t--block_size {args.block_size}",
                     f"\t--merge {args.merge}",
                     f"\t--w_rounds {args.w_rounds}",
                     f"\t--indel {args.indel}",
                     f"\t-p {args.prefix}",
                     f"\t-k {args.k}",
                     f"\t-w {args.w}",
                     f"\t-t {args.t}",
                     f"\t--fpr {args.fpr}"]), flush=True)
    if not args.no_common:
        say(f"Note: {args.prefix}.common.bf is written in btllib's Bloom filter layout as recalled from its source "
            "(header table name: --bf-signature); a stock btllib is not guaranteed to load it.")
    for fasta in fastas:
        if not os.path.isfile(fasta):
            raise FileNotFoundError(f"Input file {fasta} not found.")
    plan = ["faidx x%d" % len(fastas)] + ([] if args.no_common else ["make_common_bf"]) + \
           ["indexlr x%d" % len(fastas), "ntsynt_synteny"] + (["assess"] if args.assess else []) + (["block_identity"] if args.block_identity else []) + \
           (["block_identity_wide (edit_wide_plan, edit_wide)"] if args.block_identity and args.identity_max_edits else []) + \
           (["block_variants"] if args.block_variants else []) + \
           (["block_wide_variants (edit_script_plan, edit_script, edit_wide_script_plan, edit_wide_script)"] if args.block_wide_variants else []) + \
           (["block_ends (edit_extend, edit_extend_script_plan, edit_extend_script)" if args.block_end_variants else "block_ends (edit_extend)"]
            if args.block_ends else []) + \
           ([f"block_paf (cigar_atoms, cigar_merge{', cigar_text_scan, cigar_text_emit' if args.paf_cs else ''}; k {args.identity_k}, rate {args.identity_rate}, band {args.identity_band}, max_len {args.identity_max_len}, "
             f"max_edits {args.identity_max_edits}" + (f", ends_max_len {args.ends_max_len}, ends_max_edits {args.ends_max_edits}, ends_penalty "
                                                       f"{args.ends_penalty}" if args.block_ends else "") + ")"] if args.block_paf else []) + \
           ([f"block_chain (chain_blocks_scan, chain_blocks_emit, chain_text; k {args.identity_k}, rate {args.identity_rate}, band {args.identity_band}, "
             f"max_len {args.identity_max_len}, max_edits {args.identity_max_edits}" +
             (f", ends_max_len {args.ends_max_len}, ends_max_edits {args.ends_max_edits}, ends_penalty {args.ends_penalty}" if args.block_ends else "") + ")"]
            if args.block_chain else []) + \
           ([f"block_maf (cigar_rows_scan, cigar_rows_emit; k {args.identity_k}, rate {args.identity_rate}, band {args.identity_band}, "
             f"max_len {args.identity_max_len}, max_edits {args.identity_max_edits}" +
             (f", ends_max_len {args.ends_max_len}, ends_max_edits {args.ends_max_edits}, ends_penalty {args.ends_penalty}" if args.block_ends else "") + ")"]
            if args.block_maf else []) + \
           ([f"block_maf_multi (cigar_pad_sites, cigar_pad_emit, cigar_rows_scan, cigar_rows_emit; k {args.identity_k}, rate {args.identity_rate}, band "
             f"{args.identity_band}, max_len {args.identity_max_len}, max_edits {args.identity_max_edits}" +
             (f", ends_max_len {args.ends_max_len}, ends_max_edits {args.ends_max_edits}, ends_penalty {args.ends_penalty}" if args.block_ends else "") + ")"]
            if args.block_maf_multi else []) + \
           ([f"block_conservation (cigar_depth_events, cigar_depth_emit; k {args.identity_k}, rate {args.identity_rate}, band "
             f"{args.identity_band}, max_len {args.identity_max_len}, max_edits {args.identity_max_edits}" +
             (f", ends_max_len {args.ends_max_len}, ends_max_edits {args.ends_max_edits}, ends_penalty {args.ends_penalty}" if args.block_ends else "") + ")"]
            if args.block_conservation else []) + \
           ([f"block_variant_sites (cigar_var_bases_scan, cigar_var_bases_emit, cigar_alleles_events, cigar_alleles_emit; k {args.identity_k}, rate "
             f"{args.identity_rate}, band {args.identity_band}, max_len {args.identity_max_len}, max_edits {args.identity_max_edits}" +
             (f", ends_max_len {args.ends_max_len}, ends_max_edits {args.ends_max_edits}, ends_penalty {args.ends_penalty}" if args.block_ends else "") + ")"]
            if args.block_variant_sites else []) + \
           ([f"block_consensus (cigar_var_bases_scan, cigar_var_bases_emit, cigar_profile_events, cigar_profile_emit; k {args.identity_k}, rate "
             f"{args.identity_rate}, band {args.identity_band}, max_len {args.identity_max_len}, max_edits {args.identity_max_edits}" +
             (f", ends_max_len {args.ends_max_len}, ends_max_edits {args.ends_max_edits}, ends_penalty {args.ends_penalty}" if args.block_ends else "") + ")"]
            if args.block_consensus else []) + \
           ([f"block_lift (lift_scan, lift_search; {args.block_lift} on {args.lift_genome}; k {args.identity_k}, rate {args.identity_rate}, band "
             f"{args.identity_band}, max_len {args.identity_max_len}, max_edits {args.identity_max_edits}" +
             (f", ends_max_len {args.ends_max_len}, ends_max_edits {args.ends_max_edits}, ends_penalty {args.ends_penalty}" if args.block_ends else "") + ")"]
            if args.block_lift else []) + \
           [f"{stage} (lift_stats_scan, lift_stats_search; {what} on {args.lift_genome}; k {args.identity_k}, rate {args.identity_rate}, band "
            f"{args.identity_band}, max_len {args.identity_max_len}, max_edits {args.identity_max_edits}" +
            (f", ends_max_len {args.ends_max_len}, ends_max_edits {args.ends_max_edits}, ends_penalty {args.ends_penalty}" if args.block_ends else "") + ")"
            for stage, what, on in (("block_lift_identity", args.block_lift, args.lift_identity),
                                    ("block_windows", f"windows of {args.lift_windows}", args.lift_windows is not None)) if on] + \
           ([f"block_lift_joined (lift_pairs_scan, lift_pairs_search; " +
             " and ".join(([args.block_lift] if args.block_lift else []) + ([f"windows of {args.lift_windows}"] if args.lift_windows is not None else [])) +
             f" on {args.lift_genome}; k {args.identity_k}, rate {args.identity_rate}, band {args.identity_band}, max_len {args.identity_max_len}, "
             f"max_edits {args.identity_max_edits}" +
             (f", ends_max_len {args.ends_max_len}, ends_max_edits {args.ends_max_edits}, ends_penalty {args.ends_penalty}" if args.block_ends else "") + ")"]
            if args.lift_join else []) + \
           (["gaps"] if args.gaps else []) + \
           (["gap_links"] if args.gap_links else []) + (["gap_block_links"] if args.gap_block_links else []) + \
           (["gap_copies"] if args.gap_copies else []) + (["gap_copy_sites"] if args.gap_copy_sites else []) + \
           (["gap_periods"] if args.gap_periods else []) + (["gap_families"] if args.gap_families else [])
    if args.dry_run:
        say("Stages (GPU, in process):", " -> ".join(plan))
        return 0
    import subprocess

    def stage_failed(cause=None):
        "bin/ntSynt:166-170: a stage that stops (its message is on the terminal already) ends the run with this error, exit status 1"
        raise subprocess.SubprocessError("ntSynt failed - check the logs for the error.") from cause
    if len(args.w_rounds) != len(set(args.w_rounds)):          # stage 3's own check (bin/ntsynt_synteny.py:597-599): not under -n
        print("Error: duplicate values found in w_rounds!", file=sys.stderr, flush=True)
        stage_failed()
    from . import pipeline
    # one process per GPU under `python -m torch.distributed.run --nproc-per-node N bin/ntSynt ...`:
    # genomes are sharded over the ranks (ntsynt_amd/pipeline.py), rank 0 writes the outputs
    world = int(os.environ.get("WORLD_SIZE", "1"))
    device = args.device
    if world > 1:
        import torch
        import torch.distributed as dist
        device = int(os.environ.get("LOCAL_RANK", "0"))
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # The process group only hands the communicator id round and synchronises the ranks; the two exchanges run inside
        # libntsynt_hip.so (nts_bf_allreduce_and, nts_mx_allgather).  NTS_DIST_BACKEND=gloo + NTS_RCCL_LIB=<stand-in>: ranks that
        # share GPUs (a box with fewer GPUs than ranks; tests/test_gpu_multirank.py); production is nccl (= RCCL) throughout
        backend = os.environ.get("NTS_DIST_BACKEND", "nccl")
        if backend != "nccl":
            device %= max(torch.cuda.device_count(), 1)
        torch.cuda.set_device(device)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", device))
        else:
            dist.init_process_group(backend)
    quiet = (lambda *a, **k: None)
    try:
        _run(pipeline, fastas, args, device, quiet)
    except SystemExit as exc:                                  # a stage's own exit ("no paths found", S:630-632)
        if exc.code in (0, None):
            raise
        stage_failed()
    except Exception as exc:                                   # noqa: BLE001 -- whatever stopped a stage: its traceback is the log
        stage_failed(exc)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    if int(os.environ.get("RANK", "0")) == 0:
        print("Done ntSynt!")
    return 0


def _run(pipeline, fastas, args, device, quiet):
    lift_args = (args.lift_genome, args.identity_k, args.identity_rate, args.identity_band, args.identity_max_len, args.identity_max_edits,
                 (args.ends_max_len, args.ends_max_edits, args.ends_penalty) if args.block_ends else None)
    more = {}                                                 # (only the switches that are on: a run without them makes the call it always made)
    if args.lift_identity:
        more["block_lift_identity"] = (args.block_lift,) + lift_args
    if args.lift_windows is not None:
        more["block_windows"] = (args.lift_windows,) + lift_args
    if args.lift_join:
        more["block_lift_joined"] = lift_args
    if args.block_chain:
        more["block_chain"] = lift_args[1:]
    if args.block_maf:
        more["block_maf"] = lift_args[1:]
    if args.block_maf_multi:
        more["block_maf_multi"] = lift_args[1:]
    if args.block_conservation:
        more["block_conservation"] = lift_args[1:]
    if args.block_variant_sites:
        more["block_variant_sites"] = lift_args[1:]
    if args.block_consensus:
        more["block_consensus"] = lift_args[1:]
    pipeline.run(fastas, **more, k=args.k, w=args.w, fpr=args.fpr, prefix=args.prefix, w_rounds=args.w_rounds,
                 indel=args.indel, merge=args.merge, block_size=args.block_size, common=not args.no_common,
                 simplify=not args.no_simplify_graph, device=device, benchmark=args.benchmark,
                 dev=args.dev, interarrivals=args.interarrivals, assess=(args.assess_k, args.assess_s) if args.assess else None,
                 block_identity=((args.identity_k, args.identity_rate, args.identity_band, args.identity_max_len) + ((args.identity_max_edits,) if args.identity_max_edits else ())) if args.block_identity else None, block_variants=(args.identity_k, args.identity_rate, args.identity_band, args.identity_max_len) if args.block_variants else None, block_wide_variants=(args.identity_k, args.identity_rate, args.identity_band, args.identity_max_len, args.identity_max_edits) if args.block_wide_variants else None, block_ends=(args.ends_max_len, args.ends_max_edits, args.ends_penalty, args.identity_k, args.identity_rate, args.identity_band, args.identity_max_len, args.identity_max_edits) if args.block_ends else None, block_end_variants=args.block_end_variants, block_paf=(args.identity_k, args.identity_rate, args.identity_band, args.identity_max_len, args.identity_max_edits, (args.ends_max_len, args.ends_max_edits, args.ends_penalty) if args.block_ends else None) if args.block_paf else None, block_paf_cs=args.paf_cs, block_lift=(args.block_lift, args.lift_genome, args.identity_k, args.identity_rate, args.identity_band, args.identity_max_len, args.identity_max_edits, (args.ends_max_len, args.ends_max_edits, args.ends_penalty) if args.block_ends else None) if args.block_lift else None, gaps=args.gaps, gap_links=(args.gap_links_rate, args.gap_links_min) if args.gap_links else None, gap_block_links=args.gap_block_links, gap_copies=args.gap_links_rate if args.gap_copies else None, gap_copy_sites=(args.gap_sites_cap, args.gap_sites_step, args.gap_links_min) if args.gap_copy_sites else None, gap_periods=(args.gap_links_rate, args.gap_links_min) if args.gap_periods else None, gap_families=args.gap_sites_step if args.gap_families else None, repeat=args.repeat, bf_rounding=args.bf_rounding, bf_signature=args.bf_signature or pipeline.BF_SIGNATURE,
                 log=print if (args.dev and int(os.environ.get("RANK", "0")) == 0) else quiet)


if __name__ == "__main__":
    sys.exit(main())
