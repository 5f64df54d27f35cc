"""``tiddit`` command line on the MI355X hot path: ``python -m tiddit_amd --cov ...`` / ``--sv ...``.

Same two modes and the same flags as the reference driver (tiddit/__main__.py:22-71, :211-219).
``--cov`` is complete (byte-identical .bed/.wig for the same alignments).  ``--sv`` runs the stages this
repository implements — library statistics, signal extraction + coverage (device), GC (device), ploidy,
clustering (device) — and writes the signal ``.tab`` files, ``{o}.ploidies.tab`` and
``{o}.candidates.tab``.  By default the run stops after the candidates table and says so.

``TIDDIT_VARIANTS=1``: the scan also packs every placed record into an evidence store in HBM, and the native variant
stage (tiddit_amd/tiddit_variant.py: typing, filters, genotypes, QUAL; regional counts in one device launch over the
store) writes ``{o}.vcf`` with tiddit_amd/tiddit_vcf_header.py's header.  On N ranks every rank keeps the store of its
own shard of the file, answers all of rank 0's queries over it, and the counts are summed on rank 0, which writes the
same ``{o}.vcf``.  Local assembly stays out of scope.

``TIDDIT_COV_TRACK=Z[:Q[:bed|wig]]``: ``--sv`` also writes ``{o}.bed`` (or ``{o}.wig``), byte for byte the file ``--cov -z Z -q Q [-w]``
writes for the same BAM — from the scan's own pass over the file: the ingest kernel writes a second coverage record per read, a second
histogram is filled beside the 50-bp one, and no second job reads and inflates the file again.  On N ranks rank 0 writes it.

``TIDDIT_GENOTYPE=sites.vcf``: ``--sv`` also writes ``{o}.genotyped.vcf`` — every record of ``sites.vcf`` with this sample's
``GT:CN:COV:DV:RV:LQ:RR:DR`` (tiddit_amd/tiddit_genotype.py) — from the evidence store and the signal tables the scan left, with or
without ``TIDDIT_VARIANTS=1``.  One process only: on N ranks the switch is refused before anything is started.

``TIDDIT_DEPTH_DIST=1``: ``--sv`` also writes ``{o}.depth_dist.tab`` and ``{o}.depth_summary.tab`` — per contig and in total, the bases
covered at exactly d x and at d x or more, and the mean / min / max depth per base (tiddit_amd/tiddit_depth_dist.py) — from the evidence
store in one launch behind the candidates table.  One process only, refused on N ranks like ``TIDDIT_GENOTYPE``.

``TIDDIT_CNV=1`` (CNV bins of 500 bp) or ``TIDDIT_CNV=W`` (a multiple of 50, 50 ... 3200): ``--sv`` also writes ``{o}.cnv.bed`` — the
deletions and duplications that read depth alone shows, from an exact Viterbi segmentation of the job's coverage and GC bins on the
device behind the ploidy table (tiddit_amd/tiddit_cnv.py).  On N ranks rank 0 holds those bins and runs the stage.

``TIDDIT_ASCN=1``, only together with ``TIDDIT_CNV`` and ``TIDDIT_ALLELES``: ``--sv`` also writes ``{o}.ascn.bed`` — allele-specific copy
number: deletions, duplications, copy-neutral LOH and allelic imbalance from the CNV bins joined with the allele counters at the known
sites, by an exact 16-state Viterbi segmentation on the device behind the CNV stage (tiddit_amd/tiddit_ascn.py).  Nothing reads the BAM
again; on N ranks rank 0 holds the bins and the summed counters and runs the stage.

``TIDDIT_QC=1``: ``--sv`` also writes ``{o}.qc.tab`` — read-level QC tables from the records the scan already holds in HBM: flag counts,
MAPQ, read lengths, insert sizes, per-cycle base composition and quality, the quality histogram, GC per read, CIGAR sums and indel
lengths (tiddit_amd/tiddit_qc.py has the definition and the file's format).  Unset or empty is off; any other value ends the job with an
error before the scan.  On N ranks every rank counts the records of its shard and rank 0 writes the summed tables.

``TIDDIT_DUPS=1``: ``--sv`` also writes ``{o}.dup.tab`` — duplicate metrics recomputed from the reads' unclipped 5' ends (whatever the
file's 0x400 marks say): fragment and pair duplicates, the histogram of set sizes, the duplication rate and the estimated library size
(tiddit_amd/tiddit_dup.py has the definition and the file's format), from a key store the scan fills in HBM and one sort behind it.
Unset or empty is off; any other value ends the job with an error before the scan.  One process only, refused on N ranks like
``TIDDIT_DEPTH_DIST``: a set of duplicates can straddle a shard seam.

``TIDDIT_INDELS=1`` (minimum support 2, minimum MAPQ 20), ``TIDDIT_INDELS=S`` or ``TIDDIT_INDELS=S:Q``: ``--sv`` also writes
``{o}.indels.tab`` — every distinct insertion or deletion of 1 ... 65535 bases that at least ``S`` eligible reads (MAPQ >= ``Q``) carry in
their CIGAR, with its support by strand and the job's own 50-bp coverage bin (tiddit_amd/tiddit_indels.py has the definition and the
file's format), from a key store the scan fills in HBM and one sort behind it.  Unset or empty is off; a value that is none of the three
forms ends the job with an error before the scan.  One process only, refused on N ranks like ``TIDDIT_DUPS``: merging per-rank rows
needs an exchange of keys.

``TIDDIT_INDELS_NORM=1`` (valid only together with ``TIDDIT_INDELS``): the reference FASTA is packed into HBM before the scan
(tiddit_amd/refseq.py) and every event is left-normalised against it before its keys are made, so one indel of a repeat that reads
place differently is one row (tiddit_indels.left_normalise has the definition).  Unset or empty is off; any other value, the switch
without ``TIDDIT_INDELS``, or a contig of the BAM header that the FASTA lacks or holds at another length ends the job with an error
before the scan.

``TIDDIT_SNVS=1`` (minimum support 3, minimum MAPQ 20, minimum base quality 20), ``TIDDIT_SNVS=S``, ``S:Q`` or ``S:Q:B``: ``--sv`` also
writes ``{o}.snvs.tab`` — every position where at least ``S`` eligible reads (MAPQ >= ``Q``) carry the same base of quality >= ``B`` that
differs from the reference, with its support by strand and the job's own 50-bp coverage bin (tiddit_amd/tiddit_snvs.py has the
definition and the file's format).  The reference FASTA is packed into HBM before the scan (once, shared with ``TIDDIT_INDELS_NORM``), a
kernel compares every aligned base of every eligible read with it as the batches go by, and one sort follows the scan.  The file is a
valid ``TIDDIT_ALLELES`` sites file as it stands.  Unset or empty is off; a value that is none of the four forms, or a contig of the BAM
header that the FASTA lacks or holds at another length, ends the job with an error before the scan.  One process only, refused on N
ranks like ``TIDDIT_INDELS``.

``TIDDIT_CLIPS=1`` (minimum support 3, minimum MAPQ 20, minimum clip length 10), ``TIDDIT_CLIPS=S``, ``S:Q`` or ``S:Q:L``: ``--sv`` also
writes ``{o}.clips.tab`` — every position where at least ``S`` eligible reads (MAPQ >= ``Q``) are soft-clipped by ``L`` bases or more on
the same side, with the support by strand, a consensus of up to 28 clipped bases beside the breakpoint and the job's own 50-bp coverage
bin (tiddit_amd/tiddit_clips.py has the definition and the file's format), from a key store the scan fills in HBM, one sort and a vote
per site behind it.  Unset or empty is off; a value that is none of the four forms ends the job with an error before the scan.  One
process only, refused on N ranks like ``TIDDIT_INDELS``.

``TIDDIT_CLIPS_ALIGN=1`` (window 10000, minimum consensus columns 20, maximum mismatches 2), ``TIDDIT_CLIPS_ALIGN=W``, ``W:K`` or
``W:K:M`` (valid only together with ``TIDDIT_CLIPS``): ``--sv`` also writes ``{o}.clips.align.tab`` — for every reported clip site whose
consensus has at least ``K`` columns, the best exact placement of that consensus on the same contig within ``W`` bases of the
breakpoint, on either strand, with its mismatches (at most ``M`` for an accepted one), the number of acceptable placements, the event
the junction implies (DEL / DUP / INV and its length, base-pair exact) and the opposite-side site that tells the same event with the
microhomology between the two (tiddit_amd/tiddit_clip_align.py has the definition and the file's format).  The reference FASTA is packed
into HBM before the scan (once, shared with ``TIDDIT_INDELS_NORM`` / ``TIDDIT_SNVS``) and one kernel searches it behind the clip stage's
finish, on the site rows where they lie.  ``{o}.clips.tab`` and every other output are what they are without the switch.  Unset or
empty is off; the switch without ``TIDDIT_CLIPS``, a value that is none of the four forms, or a contig of the BAM header that the FASTA
lacks or holds at another length, ends the job with an error before the scan.

``TIDDIT_CLIPS_FAR=1`` (minimum consensus columns 20, maximum mismatches 2), ``TIDDIT_CLIPS_FAR=K`` or ``K:M`` (valid only together with
``TIDDIT_CLIPS``; independent of ``TIDDIT_CLIPS_ALIGN``: either, both or neither): ``--sv`` also writes ``{o}.clips.far.tab`` — for every
reported clip site whose consensus has at least ``K`` columns (16 ... 28), the best placement of that consensus on ANY contig of the
reference, on either strand, whose first 16 columns match exactly and whose other columns differ in at most ``M`` places (0 ... 12),
with the number of such placements, the event the junction implies (BND on another contig; REF / DEL / DUP / INV on the site's own) and
the opposite-side site that tells the same junction with the microhomology between the two (tiddit_amd/tiddit_clip_far.py has the
definition and the file's format): translocations, dispersed duplications and clips that place many times, which the window of
``TIDDIT_CLIPS_ALIGN`` cannot reach.  The reference is packed into HBM before the scan (once, shared with the other switches that read
it) and streams once against a sorted seed table of the sites behind the clip stage's finish.  Every other output is what it is
without the switch.  Unset or empty is off; the switch without ``TIDDIT_CLIPS``, a value that is none of the three forms, or a contig of
the BAM header that the FASTA lacks or holds at another length, ends the job with an error before the scan.

``TIDDIT_CLIPS_INS=1`` (minimum extended-consensus columns 20, minimum overlap 12, maximum mismatches 1), ``TIDDIT_CLIPS_INS=K``, ``K:O``
or ``K:O:M`` (valid only together with ``TIDDIT_CLIPS``; independent of ``TIDDIT_CLIPS_ALIGN`` and ``TIDDIT_CLIPS_FAR``, and no FASTA goes
into HBM for it): ``--sv`` also writes ``{o}.clips.ins.tab`` — insertion candidates from clip sites that face each other.  The vote over
the clipped bases of a site is carried from 28 to 140 columns (a second key store beside the first, one more launch per batch), every
``R`` site with at least ``K`` (10 ... 140) columns is paired with every such ``L`` site at ``P_R + 1`` or up to 32 bases to its left (a
target-site duplication), and the pair is ``CLOSED`` where the two extended consensus overlap by ``O`` (8 ... 140) bases or more with at
most ``M`` (0 ... 8) mismatches, with the inserted sequence (up to 2 x 140 - ``O`` bases); otherwise it is ``OPEN`` and the two flanks
are what is known of a longer insertion (tiddit_amd/tiddit_clip_ins.py has the definition and the file's format).  Every other output is
what it is without the switch.  Unset or empty is off; the switch without ``TIDDIT_CLIPS``, or a value that is none of the four forms,
ends the job with an error before the scan.  N ranks are refused with ``TIDDIT_CLIPS``.

``TIDDIT_CLIPS_VCF=1`` (flank 10) or ``TIDDIT_CLIPS_VCF=F`` (2 ... 1000; valid only together with ``TIDDIT_CLIPS`` and at least one of
``TIDDIT_CLIPS_ALIGN`` / ``TIDDIT_CLIPS_FAR`` / ``TIDDIT_CLIPS_INS``): ``--sv`` also writes ``{o}.clips.vcf`` — the mated DEL / DUP / BND rows of
the two placement stages as one record per junction (a BND two), left-aligned through the microhomology, and the insertion pairs that
no junction explains, each with a genotype from the clipped reads at its two sites against the reads that cross either breakpoint
intact with ``F`` aligned bases on both sides (tiddit_amd/tiddit_clip_vcf.py has the definition and the file's format).  The scan keeps
its evidence store as for ``TIDDIT_DEPTH_DIST``, and one launch behind the clip stages counts all breakpoints over it where it lies; the
store is neither taken nor freed.  Every other output is what it is without the switch.  A bare ``1`` means the default, so a flank of
1 cannot be asked for.  Unset or empty is off; the switch without its partners, or any other value, ends the job with an error before
the scan.  N ranks are refused with ``TIDDIT_CLIPS``.

``TIDDIT_CLIPS_MEI=library.fa`` (valid only together with ``TIDDIT_CLIPS`` and ``TIDDIT_CLIPS_INS``) and ``TIDDIT_CLIPS_MEI_MIN=A``
(12 ... 280, default 30; valid only with it): ``--sv`` also writes ``{o}.clips.mei.tab`` — every sequence of ``{o}.clips.ins.tab`` (a
``CLOSED`` pair's ``SEQ``, an ``OPEN`` pair's two flanks) aligned with gaps to every sequence of the library (1 ... 4096 sequences,
2^20 bases in all: family consensus such as Alu, L1, SVA, HERV-K) on both strands, with the best family, its strand, score and spans
where the score is at least ``A`` (tiddit_amd/tiddit_clip_mei.py has the definition and the file's format).  The library is packed
into HBM behind the scan, in a handle of its own, and freed behind the stage.  With ``TIDDIT_CLIPS_VCF`` the ``<INS>`` records of the
named pairs gain ``MEI`` / ``MEISTRAND`` / ``MEISCORE`` / ``MEISPAN``; every other output is what it is without the switch.  Unset or
empty is off; a file that cannot be read, a library outside the limits, the switch without its partners, ``TIDDIT_CLIPS_MEI_MIN``
without the switch or out of range ends the job with an error before the scan.  N ranks are refused with ``TIDDIT_CLIPS``.
"""
import argparse
import os
import sys
import time


def _sv_parser():
    p = argparse.ArgumentParser("""tiddit --sv --bam inputfile [-o prefix] --ref ref.fasta""")
    p.add_argument("--sv", help="call structural variation", required=False, action="store_true")
    p.add_argument("--force_overwrite", help="force the analysis and overwrite any data in the output folder", required=False, action="store_true")
    p.add_argument("--bam", type=str, required=True, help="coordinate sorted bam file(required)")
    p.add_argument("--ref", type=str, help="reference fasta", required=True)
    p.add_argument("-o", type=str, default="output", help="output prefix(default=output)")
    p.add_argument("-i", type=int, help="paired reads maximum allowed insert size (default= 99.9th percentile of insert size)")
    p.add_argument("-d", type=str, help="expected reads orientations, possible values \"innie\" (-> <-) or \"outtie\" (<- ->)")
    p.add_argument("-p", type=int, default=3, help="Minimum number of supporting pairs in order to call a variant (default 3)")
    p.add_argument("--threads", type=int, default=1, help="Number of threads (default=1)")
    p.add_argument("-r", type=int, default=3, help="Minimum number of supporting split reads to call a variant (default 3)")
    p.add_argument("-q", type=int, default=5, help="Minimum mapping quality to consider an alignment (default 5)")
    p.add_argument("-n", type=int, default=2, help="the ploidy of the organism,(default = 2)")
    p.add_argument("-e", type=int, help="clustering distance parameter (default = half the average insert size)")
    p.add_argument("-c", type=float, help="average coverage, overwrites the estimated average coverage")
    p.add_argument("-l", type=int, default=3, help="min-pts parameter (default=3),must be set >= 2")
    p.add_argument("-s", type=int, default=25000000, help="Number of reads to sample when computing library statistics(default=25000000)")
    p.add_argument("--force_ploidy", action="store_true", help="force the ploidy to be set to -n across the entire genome")
    p.add_argument("--n_mask", type=float, default=0.5, help="exclude regions from coverage calculation if they contain more than this fraction of N (default = 0.5)")
    p.add_argument("--p_ratio", type=float, default=0.1, help="minimum discordant pair/normal pair ratio at the breakpoint junction(default=0.1)")
    p.add_argument("--r_ratio", type=float, default=0.1, help="minimum split read/coverage ratio at the breakpoint junction(default=0.1)")
    p.add_argument("--max_coverage", type=float, default=4, help="filter call if X times higher than chromosome average coverage (default=4)")
    p.add_argument("--min_contig", type=int, default=10000, help="Skip calling on small contigs (default < 10000 bp)")
    p.add_argument("-z", type=int, default=50, help="minimum variant size (default=50)")
    p.add_argument("--skip_assembly", action="store_true", help="Skip running local assembly")
    p.add_argument("--bwa", type=str, default="bwa", help="path to bwa executable file(default=bwa)")
    p.add_argument("--min_clip", type=int, default=4, help="Minimum clip reads to initiate local assembly of a region(default=4)")
    p.add_argument("--padding", type=int, default=100, help="Extend the local assembly by this number of bases (default=100bp)")
    p.add_argument("--min_pts_clips", type=int, default=3, help="min-pts parameter for the clustering of candidates for local assembly (default=3)")
    p.add_argument("--max_assembly_reads", type=int, default=100000, help="Skip assembly of regions containing too many reads")
    p.add_argument("--max_local_assembly_region", type=int, default=2000, help="maximum size of the clip read cluster for local assembly")
    p.add_argument("--min_anchor_len", type=int, default=60, help="minimum mapped bases to be considered a clip read  (default=60 bp)")
    p.add_argument("--min_clip_len", type=int, default=25, help="minimum clipped bases to be considered a clip read (default=25 bp)")
    p.add_argument("--min_contig_len", type=int, default=200, help="minimum contig length for SV analysis (default=200 bp)")
    p.add_argument("-k", type=int, default=91, help="kmer lenght used by the local assembler (default=91 bp)")
    return p


def _cov_parser():
    p = argparse.ArgumentParser("""tiddit --cov --bam inputfile [-o prefix]""")
    p.add_argument("--cov", help="generate a coverage bed/wig file", required=False, action="store_true")
    p.add_argument("--bam", type=str, required=True, help="coordinate sorted bam file(required)")
    p.add_argument("-o", type=str, default="output", help="output prefix(default=output)")
    p.add_argument("-z", type=int, default=500, help="use bins of specified size(default = 500bp) to measure the coverage of the entire bam file")
    p.add_argument("-w", help="generate wig instead of bed", required=False, action="store_true")
    p.add_argument("-q", type=int, help="minimum mapping quality(default=20)", required=False, default=20)
    p.add_argument("--ref", type=str, help="reference fasta, used for reading cram")
    return p


def run_cov(args):
    from . import tiddit_coverage
    from .bamio import DeviceBatch, open_bam
    if not os.path.isfile(args.bam):
        print("error,  could not find the bam file")
        quit()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:                                                      # one process per GPU on ONE file: sharded ingest + all-reduce
        import torch
        import torch.distributed as dist
        from . import dist as tdist
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        if not dist.is_initialized():
            dist.init_process_group("nccl")
        bam_header, coverage_data, _ = tdist.coverage_sharded(args.bam, args.z, args.q)
        if dist.get_rank() != 0:
            return
    else:
        reader = open_bam(args.bam)                                        # inflate + record decode on the device by default
        bam_header = reader.header
        coverage_data, end_bin_size = tiddit_coverage.create_coverage(bam_header, args.z)
        hist = tiddit_coverage.CoverageHistogram(bam_header, args.z)
        if hasattr(reader, "bin_for"):
            reader.bin_for(hist)                 # the ingest kernel writes the coverage records for this bin size
        import numpy
        for b in reader.batches():
            if isinstance(b, DeviceBatch):
                hist.push_device_batch(b, args.q)
                reader.ahead()                   # (the launch reads the batch's coverage records, not its raw bytes: the next span's inflate may follow it)
                continue
            tid = b.tid
            edges = numpy.flatnonzero(numpy.diff(tid)) + 1
            for lo, hi in zip(numpy.concatenate([[0], edges]), numpy.concatenate([edges, [len(tid)]])):
                if tid[lo] >= 0:
                    hist.push(int(tid[lo]), b.pos[lo:hi], b.end[lo:hi], b.mapq[lo:hi], b.flag[lo:hi], args.q)
        reader.close()
        # (a header of thousands of contigs: every contig's bins in one launch + copy, tdt_cov_finish_all; contigs are found by name)
        coverage_data.update(tiddit_coverage.bins_by_contig(hist, coverage_data))
        hist.close()
    if args.w:
        tiddit_coverage.print_coverage(coverage_data, bam_header, args.z, "wig", args.o + ".wig")
    else:
        tiddit_coverage.print_coverage(coverage_data, bam_header, args.z, "bed", args.o + ".bed")


def parse_cov_track(value):
    """``TIDDIT_COV_TRACK``: ``Z[:Q[:bed|wig]]`` -> (bin size, minimum mapping quality, file type), with the defaults of ``--cov``
    (-q 20, bed); None when the switch is unset or empty.  Raises ValueError (its text is the error line) for anything else."""
    if value is None or value == "":
        return None
    fields = value.split(":")
    if len(fields) > 3:
        raise ValueError("at most three fields, Z[:Q[:bed|wig]]")
    import re
    if not re.fullmatch(r"[0-9]+", fields[0]) or (len(fields) > 1 and not re.fullmatch(r"-?[0-9]+", fields[1])):
        raise ValueError("the bin size and the mapping quality are integers")
    z = int(fields[0])
    q = int(fields[1]) if len(fields) > 1 else 20
    if z < 1:
        raise ValueError("the bin size must be at least 1")
    fmt = fields[2] if len(fields) > 2 else "bed"
    if fmt not in ("bed", "wig"):
        raise ValueError("the file type is bed or wig")
    return z, q, fmt


STAGE_SECONDS = {}          # wall seconds of the last run_sv, stage by stage (bench.py reads it)
STAGE_NOTES = {}            # ... and counts that are not seconds


def write_candidates(path, contigs, sv_clusters):
    with open(path, "w") as f:
        f.write("#chrA\tposA\tchrB\tposB\tcluster\tN_discordants\tN_splits\tN_contigs\tstartA\tendA\tstartB\tendB\n")
        for chrA in contigs:
            if chrA not in sv_clusters:
                continue
            for chrB in sv_clusters[chrA]:
                for cid, c in sv_clusters[chrA][chrB].items():
                    f.write("\t".join(map(str, [chrA, c["posA"], chrB, c["posB"], cid, c["N_discordants"], c["N_splits"], c["N_contigs"],
                                                c["startA"], c["endA"], c["startB"], c["endB"]])) + "\n")


def variant_stage(tiddit_variant, tiddit_vcf_header, prefix, contigs, bam_header, library, sample_id, version, args, sv_clusters, min_mapq, samples,
                  coverage_data, contig_number, max_ins_len, gc_dictionary, entry=None):
    """the tail of the reference's driver (__main__.py:193-207) with the two modules handed in: header, variants per contig sorted by
    position, {prefix}.vcf.  entry: the variant module's function to call (default its ``main``; on N ranks every rank calls
    ``main_sharded``, and the ranks it returns None on write nothing).  -> False (nothing written) when the reference package is
    not there, or on a rank that does not write."""
    if tiddit_variant is None or tiddit_vcf_header is None:
        return False
    variants = (entry or tiddit_variant.main)(args.bam, sv_clusters, args, library, min_mapq, samples, coverage_data, contig_number,
                                              max_ins_len, gc_dictionary)
    if variants is None:
        return False
    vcf_header = tiddit_vcf_header.main(bam_header, library, sample_id, version)
    with open(prefix + ".vcf", "w") as f:
        f.write(vcf_header + "\n")
        for chrom in contigs:
            if chrom not in variants:
                continue
            for variant in sorted(variants[chrom], key=lambda x: x[0]):
                f.write("\t".join(variant[1]) + "\n")
    return True


def run_sv(args, version):
    """``tiddit --sv``; the switches of the scan are documented at the head of this file, and one more here.

    ``TIDDIT_STR=loci.bed`` with ``TIDDIT_STR_CUTS=F``, ``F:S`` or ``F:S:Q`` (flank 5, minimum spanning reads 5, minimum MAPQ 20; valid only
    with ``TIDDIT_STR``): ``--sv`` also writes ``{o}.str.tab`` — for every locus of a tab-separated catalogue ``chrom start end motif [id]``
    (0-based half-open, plain or gzip, motifs of 1 to 6 bases) the repeat lengths the eligible reads (MAPQ >= ``Q``) show between its two
    neighbour bases with ``F`` aligned bases on both sides, a genotype where at least ``S`` reads span it, and how far reads that end inside
    the repeat keep repeating the motif — through soft clips — with a flag where that is longer than any spanning read shows
    (tiddit_amd/tiddit_str.py has the definition and the file's format), from a key store the scan fills in HBM and one sort behind it.  No
    second pass over the BAM, no reference in HBM.  Unset or empty is off; a file that cannot be read, cuts of another form, or the cuts
    without the switch end the job with an error before the scan.  One process only, refused on N ranks like ``TIDDIT_INDELS``.
    """
    from . import tiddit_cluster, tiddit_coverage_analysis, tiddit_gc, tiddit_signal, tiddit_stats
    from .bamio import BamReader
    from .fasta import FastaFile
    if args.l < 2:
        print("error, too low --l value!")
        quit()
    try:
        track = parse_cov_track(os.environ.get("TIDDIT_COV_TRACK"))
    except ValueError as e:
        print("error, TIDDIT_COV_TRACK={}: {}".format(os.environ.get("TIDDIT_COV_TRACK"), e))
        quit()
    try:
        from . import tiddit_depth_dist
        depth_dist = tiddit_depth_dist.parse_switch(os.environ.get("TIDDIT_DEPTH_DIST"))
    except ValueError as e:
        # (before anything is read or made: no {o}_tiddit is left behind)
        print("error, TIDDIT_DEPTH_DIST={}: {}".format(os.environ.get("TIDDIT_DEPTH_DIST"), e))
        sys.exit(1)
    try:
        from . import tiddit_cnv
        cnv = tiddit_cnv.parse_switch(os.environ.get("TIDDIT_CNV"))
    except ValueError as e:
        # (the same)
        print("error, TIDDIT_CNV={}: {}".format(os.environ.get("TIDDIT_CNV"), e))
        sys.exit(1)
    try:
        from . import tiddit_alleles
        alleles = tiddit_alleles.parse_switch(os.environ.get("TIDDIT_ALLELES"), os.environ.get("TIDDIT_ALLELES_MIN_BQ"))
    except ValueError as e:
        # (the same)
        print("error, TIDDIT_ALLELES={}: {}".format(os.environ.get("TIDDIT_ALLELES"), e))
        sys.exit(1)
    try:
        from . import tiddit_ascn
        ascn = tiddit_ascn.parse_switch(os.environ.get("TIDDIT_ASCN"), cnv, alleles)
    except ValueError as e:
        # (the same)
        print("error, TIDDIT_ASCN={}: {}".format(os.environ.get("TIDDIT_ASCN"), e))
        sys.exit(1)
    try:
        # TIDDIT_PHASE=1 | S | S:H, only together with TIDDIT_ALLELES: read-backed phasing of the heterozygous sites of the sites file
        # ({o}.phase.tab, {o}.phase.blocks.tab; tiddit_phase.py is the specification and documents the switch)
        from . import tiddit_phase
        phase = tiddit_phase.parse_switch(os.environ.get("TIDDIT_PHASE"), alleles is not None)
    except ValueError as e:
        # (the same)
        print("error, TIDDIT_PHASE={}: {}".format(os.environ.get("TIDDIT_PHASE"), e))
        sys.exit(1)
    try:
        from . import tiddit_qc
        qc = tiddit_qc.parse_switch(os.environ.get("TIDDIT_QC"))
    except ValueError as e:
        # (the same)
        print("error, TIDDIT_QC={}: {}".format(os.environ.get("TIDDIT_QC"), e))
        sys.exit(1)
    try:
        from . import tiddit_dup
        dups = tiddit_dup.parse_switch(os.environ.get("TIDDIT_DUPS"))
    except ValueError as e:
        # (the same)
        print("error, TIDDIT_DUPS={}: {}".format(os.environ.get("TIDDIT_DUPS"), e))
        sys.exit(1)
    try:
        from . import tiddit_indels
        indels = tiddit_indels.parse_switch(os.environ.get("TIDDIT_INDELS"))
    except ValueError as e:
        # (the same)
        print("error, TIDDIT_INDELS={}: {}".format(os.environ.get("TIDDIT_INDELS"), e))
        sys.exit(1)
    try:
        indels_norm = tiddit_indels.parse_norm_switch(os.environ.get("TIDDIT_INDELS_NORM"), indels)
    except ValueError as e:
        # (the same)
        print("error, TIDDIT_INDELS_NORM={}: {}".format(os.environ.get("TIDDIT_INDELS_NORM"), e))
        sys.exit(1)
    try:
        from . import tiddit_str
        strs = tiddit_str.parse_switch(os.environ.get("TIDDIT_STR"), os.environ.get("TIDDIT_STR_CUTS"))
    except ValueError as e:
        # (the same)
        print("error, TIDDIT_STR_CUTS={}: {}".format(os.environ.get("TIDDIT_STR_CUTS"), e))
        sys.exit(1)
    try:
        from . import tiddit_snvs
        snvs = tiddit_snvs.parse_switch(os.environ.get("TIDDIT_SNVS"))
    except ValueError as e:
        # (the same)
        print("error, TIDDIT_SNVS={}: {}".format(os.environ.get("TIDDIT_SNVS"), e))
        sys.exit(1)
    try:
        from . import tiddit_small_vcf
        small_vcf = tiddit_small_vcf.parse_switch(os.environ.get("TIDDIT_SMALL_VCF"), snvs, indels)
    except ValueError as e:
        # (the same)
        print("error, TIDDIT_SMALL_VCF={}: {}".format(os.environ.get("TIDDIT_SMALL_VCF"), e))
        sys.exit(1)
    try:
        from . import tiddit_clips
        clips = tiddit_clips.parse_switch(os.environ.get("TIDDIT_CLIPS"))
    except ValueError as e:
        # (the same)
        print("error, TIDDIT_CLIPS={}: {}".format(os.environ.get("TIDDIT_CLIPS"), e))
        sys.exit(1)
    try:
        from . import tiddit_clip_align
        clips_align = tiddit_clip_align.parse_switch(os.environ.get("TIDDIT_CLIPS_ALIGN"), clips is not None)
    except ValueError as e:
        # (the same)
        print("error, TIDDIT_CLIPS_ALIGN={}: {}".format(os.environ.get("TIDDIT_CLIPS_ALIGN"), e))
        sys.exit(1)
    try:
        from . import tiddit_clip_far
        clips_far = tiddit_clip_far.parse_switch(os.environ.get("TIDDIT_CLIPS_FAR"), clips is not None)
    except ValueError as e:
        # (the same)
        print("error, TIDDIT_CLIPS_FAR={}: {}".format(os.environ.get("TIDDIT_CLIPS_FAR"), e))
        sys.exit(1)
    try:
        from . import tiddit_clip_ins
        clips_ins = tiddit_clip_ins.parse_switch(os.environ.get("TIDDIT_CLIPS_INS"), clips is not None)
    except ValueError as e:
        # (the same)
        print("error, TIDDIT_CLIPS_INS={}: {}".format(os.environ.get("TIDDIT_CLIPS_INS"), e))
        sys.exit(1)
    try:
        from . import tiddit_clip_mei
        clips_mei = tiddit_clip_mei.parse_switch(os.environ.get("TIDDIT_CLIPS_MEI"), os.environ.get("TIDDIT_CLIPS_MEI_MIN"), clips is not None,
                                                 clips_ins is not None)
    except ValueError as e:
        # (the same)
        _var = "TIDDIT_CLIPS_MEI" if os.environ.get("TIDDIT_CLIPS_MEI") else "TIDDIT_CLIPS_MEI_MIN"
        print("error, {}={}: {}".format(_var, os.environ.get(_var), e))
        sys.exit(1)
    try:
        from . import tiddit_clip_vcf
        clips_vcf = tiddit_clip_vcf.parse_switch(os.environ.get("TIDDIT_CLIPS_VCF"), clips is not None,
                                                 clips_align is not None or clips_far is not None or clips_ins is not None)
    except ValueError as e:
        # (the same)
        print("error, TIDDIT_CLIPS_VCF={}: {}".format(os.environ.get("TIDDIT_CLIPS_VCF"), e))
        sys.exit(1)
    sites_path = os.environ.get("TIDDIT_GENOTYPE") or None
    genotype_depth = os.environ.get("TIDDIT_GENOTYPE_DEPTH") == "1"
    if genotype_depth and sites_path is None:
        # (before anything is read or made: no {o}_tiddit is left behind)
        print("error, TIDDIT_GENOTYPE_DEPTH=1 annotates the sites of TIDDIT_GENOTYPE=sites.vcf, which is not set")
        sys.exit(1)
    if not args.skip_assembly:
        print("error, local assembly is outside this build's scope; rerun with --skip_assembly")
        quit()
    if not os.path.isfile(args.ref):
        print("error,  could not find the reference file")
        quit()
    FastaFile(args.ref)          # builds ref.fai when it is missing (pysam.faidx in the reference)
    if not (args.bam.endswith(".bam") or args.bam.endswith(".cram")):
        print("error, the input file is not a bam file, make sure that the file extension is .bam or .cram")
        quit()
    if args.bam.endswith(".cram"):
        print("error, CRAM input is not supported by this build (BAM only)")
        quit()
    if not os.path.isfile(args.bam):
        print("error,  could not find the bam file")
        quit()
    reader = BamReader(args.bam, batch_bytes=1 << 20)    # (the header only: small pieces — the default piece inflates 3-4 ms of blocks nobody reads)
    bam_header = reader.header
    reader.close()
    chromosomes = [c["SN"] for c in bam_header["SQ"]]
    try:
        sample_id = bam_header["RG"][0]["SM"]
    except Exception:
        sample_id = args.bam.split("/")[-1].split(".")[0]
    samples = [sample_id]
    contigs = list(chromosomes)
    contig_number = {c: i for i, c in enumerate(contigs)}
    contig_length = {c["SN"]: c["LN"] for c in bam_header["SQ"]}
    prefix = args.o
    if indels_norm or snvs is not None or small_vcf is not None or clips_align is not None or clips_far is not None:
        # TIDDIT_INDELS_NORM / TIDDIT_SNVS / TIDDIT_SMALL_VCF / TIDDIT_CLIPS_ALIGN / TIDDIT_CLIPS_FAR: the contigs of the BAM header are matched to the
        # FASTA's by name now — one that is missing or has another length ends the job before anything is made
        from . import refseq
        norm_fasta = FastaFile(args.ref)
        try:
            refseq.check_against_bam(norm_fasta, chromosomes, [contig_length[c] for c in chromosomes])
        except ValueError as e:
            if indels_norm:
                print("error, TIDDIT_INDELS_NORM=1: {}".format(e))
            elif snvs is not None:
                print("error, TIDDIT_SNVS={}: {}".format(os.environ.get("TIDDIT_SNVS"), e))
            elif small_vcf is not None:
                print("error, TIDDIT_SMALL_VCF=1: {}".format(e))
            elif clips_align is not None:
                print("error, TIDDIT_CLIPS_ALIGN={}: {}".format(os.environ.get("TIDDIT_CLIPS_ALIGN"), e))
            else:
                print("error, TIDDIT_CLIPS_FAR={}: {}".format(os.environ.get("TIDDIT_CLIPS_FAR"), e))
            sys.exit(1)
    allele_sites = None
    if alleles is not None:
        # TIDDIT_ALLELES: the sites are read now, on every rank — a file that cannot be read ends the job before anything is made
        t_sites = time.time()
        try:
            allele_sites = tiddit_alleles.read_sites(alleles[0], chromosomes, [contig_length[c] for c in chromosomes])
        except (OSError, EOFError, UnicodeDecodeError) as e:
            print("error, TIDDIT_ALLELES={}: {}".format(alleles[0], e))
            sys.exit(1)
        t_sites = time.time() - t_sites
    str_loci = None
    if strs is not None:
        # TIDDIT_STR: the loci are read now, on every rank — a file that cannot be read ends the job before anything is made
        t_loci = time.time()
        try:
            str_loci = tiddit_str.read_loci(strs[0], chromosomes, [contig_length[c] for c in chromosomes])
        except (OSError, EOFError, UnicodeDecodeError) as e:
            print("error, TIDDIT_STR={}: {}".format(strs[0], e))
            sys.exit(1)
        t_loci = time.time() - t_loci
    # one process per GPU on ONE file (BASELINE configs[4]; `torchrun --nproc-per-node N -m tiddit_amd --sv ...`): rank 0 owns the
    # output files and the host-only stages, the signal scan and the clustering are shared (tiddit_signal.main_sharded,
    # tiddit_cluster.main_sharded)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = 0
    dist = None
    # TIDDIT_FORCE_DIST=1: take the N-rank code path with whatever WORLD_SIZE says, also 1 — a one-GPU box can then run every
    # collective of the job over real RCCL (backend nccl refuses two ranks on one device; tests/test_gpu_sv_e2e.py)
    multi = world > 1 or os.environ.get("TIDDIT_FORCE_DIST") == "1"
    if multi and sites_path is not None:
        # (every rank, before the first collective: no rank is left waiting for another)
        print("error, TIDDIT_GENOTYPE is a one-process switch: the N-rank job (WORLD_SIZE > 1 or TIDDIT_FORCE_DIST=1) does not genotype sites")
        sys.exit(1)
    if multi and depth_dist:
        # (the same: a base near a shard seam is covered by two shards' reads, and per-shard histograms of depth do not add up)
        print("error, TIDDIT_DEPTH_DIST is a one-process switch: the N-rank job (WORLD_SIZE > 1 or TIDDIT_FORCE_DIST=1) holds every shard's "
              "reads on another rank")
        sys.exit(1)
    if multi and dups:
        # (the same: a set of duplicates can straddle a shard seam, and per-rank set counts do not add up)
        print("error, TIDDIT_DUPS is a one-process switch: the N-rank job (WORLD_SIZE > 1 or TIDDIT_FORCE_DIST=1) holds every shard's "
              "keys on another rank")
        sys.exit(1)
    if multi and phase is not None:
        # (the same: a fragment's two mates can lie on two shards, and its link would be lost.  TIDDIT_ALLELES alone stays allowed)
        print("error, TIDDIT_PHASE is a one-process switch: the N-rank job (WORLD_SIZE > 1 or TIDDIT_FORCE_DIST=1) holds every shard's "
              "keys on another rank")
        sys.exit(1)
    if multi and small_vcf is not None:
        # (the same, in front of its partners' refusals: a base near a shard seam is covered by two shards' reads)
        print("error, TIDDIT_SMALL_VCF is a one-process switch: the N-rank job (WORLD_SIZE > 1 or TIDDIT_FORCE_DIST=1) holds every shard's "
              "reads on another rank")
        sys.exit(1)
    if multi and indels is not None:
        # (the same: an event's support is spread over the shards, and merging per-rank rows needs an exchange of keys)
        print("error, TIDDIT_INDELS is a one-process switch: the N-rank job (WORLD_SIZE > 1 or TIDDIT_FORCE_DIST=1) holds every shard's "
              "keys on another rank")
        sys.exit(1)
    if multi and strs is not None:
        # (the same: a locus's reads are spread over the shards)
        print("error, TIDDIT_STR is a one-process switch: the N-rank job (WORLD_SIZE > 1 or TIDDIT_FORCE_DIST=1) holds every shard's "
              "keys on another rank")
        sys.exit(1)
    if multi and snvs is not None:
        # (the same: a set of equal keys can straddle the shards)
        print("error, TIDDIT_SNVS is a one-process switch: the N-rank job (WORLD_SIZE > 1 or TIDDIT_FORCE_DIST=1) holds every shard's "
              "keys on another rank")
        sys.exit(1)
    if multi and clips is not None:
        # (the same: a site's keys can straddle the shards)
        print("error, TIDDIT_CLIPS is a one-process switch: the N-rank job (WORLD_SIZE > 1 or TIDDIT_FORCE_DIST=1) holds every shard's "
              "keys on another rank")
        sys.exit(1)
    if multi:
        import torch
        import torch.distributed as dist
        from . import dist as tdist
        backend = os.environ.get("TIDDIT_DIST_BACKEND", "nccl")          # gloo: ranks sharing one GPU (tests)
        if backend == "nccl":
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        own_group = not dist.is_initialized()
        if own_group:
            dist.init_process_group(backend)
        rank = dist.get_rank()
    if rank == 0:
        try:
            os.mkdir("{}_tiddit".format(prefix))
            os.mkdir("{}_tiddit/clips".format(prefix))
        except Exception:
            if not args.force_overwrite:
                print("Eror output folder exists")
                if multi:
                    dist.destroy_process_group()
                    os._exit(1)                                          # (the other ranks sit in the broadcast below: take the job down)
                quit()
    min_mapq = args.q
    max_ins_len = 100000
    T = STAGE_SECONDS
    T.clear()
    STAGE_NOTES.clear()
    if allele_sites is not None:
        T["allele sites (host, before the scan)"] = t_sites
    from .trace import stage
    # The GC / N-mask bins depend on the reference FASTA alone (the reference computes them after the signals, __main__.py:166): a
    # second host thread with its own library context (own streams and scratch) reads the FASTA and runs the GC kernel BESIDE the BAM
    # scan — the scan waits inside the library (inflate-kernel bound; its row path holds no Python since round 4), so the thread's
    # short Python moments cost it nothing, and 3 GB more over a link that carries 54 GB in 2.2 s are noise.  (While the rows were
    # Python objects the thread started behind the scan, tiddit_signal.AFTER_SCAN, because the two fought over the GIL: that left
    # 0.42 s of a 3-Gb job waiting for it.)  On N ranks every rank computes the bins of ITS contigs (dist.shard_contigs) and rank 0
    # receives them.  TIDDIT_GC_OVERLAP=0: in sequence on rank 0's main thread; =after: the thread starts when the scan is over.
    gc_job = None
    gc_mode = os.environ.get("TIDDIT_GC_OVERLAP", "1")
    if gc_mode != "0":
        import threading
        from . import _native
        gc_job = {}
        gc_mine = list(chromosomes)
        if multi:
            owned = tdist.shard_contigs([contig_length[c] for c in chromosomes], world)[rank]
            gc_mine = [chromosomes[i] for i in owned]

        def gc_thread():
            try:
                ctx = _native.Context(_native.default_context().device)
                fasta = FastaFile(args.ref)
                gc_job["result"] = tiddit_gc.gc_of_contigs(fasta, gc_mine, 50, 0.5, ctx=ctx)
            except BaseException as e:           # re-raised on the main thread
                gc_job["error"] = e
            gc_job["seconds"] = time.time() - gc_job["t0"]

        def start_gc():
            if "thread" not in gc_job:
                gc_job["t0"] = time.time()
                gc_job["thread"] = threading.Thread(target=gc_thread, name="tiddit-gc")
                gc_job["thread"].start()
        if gc_mode == "after":
            tiddit_signal.AFTER_SCAN.append(start_gc)
        elif not multi and gc_mode != "scan":
            start_gc()          # one process: now, beside the statistics pass too (started behind it, a 240-Mb job — 0.06 s of scan for 0.055 s of GC
                                # thread — waited 3-24 ms for the thread at its end; TIDDIT_GC_OVERLAP=scan starts it behind the statistics as before)
    t = time.time()
    with stage("tiddit: library statistics"):
        if not multi:
            try:
                library = tiddit_stats.statistics(args.bam, args.ref, min_mapq, max_ins_len, args.s, carry=True,
                                                     **({} if track is None else {"track_bin_size": track[0]}))
            except BaseException:
                if gc_job is not None and "thread" in gc_job:
                    gc_job["thread"].join()                  # (no helper thread outlives the error)
                raise
        else:
            # The sample is the head of the file = the head of rank 0's byte range: rank 0 samples it through its own share's reader and
            # keeps the batches for its scan.  Nothing in inflate / record decode / the coverage records depends on the statistics, so the
            # other ranks do not wait idle for the broadcast: they ingest the head of THEIR shares meanwhile (bamio.preingest) and their
            # scans start from those batches.  TIDDIT_DIST_PREINGEST=0: wait idle (what the first N-rank build did).
            import pickle
            import numpy
            from . import bamio
            wire = torch.zeros(8192, dtype=torch.uint8, device=tdist._wire_device())
            overlap = os.environ.get("TIDDIT_DIST_PREINGEST", "1") != "0" and os.environ.get("TIDDIT_HOST_INGEST") != "1"
            if rank == 0:
                library = tiddit_stats.statistics(args.bam, args.ref, min_mapq, max_ins_len, args.s, carry=overlap, shard=(0, world) if overlap else None,
                                                     **({} if track is None else {"track_bin_size": track[0]}))
                blob = pickle.dumps(library, protocol=4)
                host = numpy.zeros(8192, dtype=numpy.uint8)
                big = len(blob) > host.size - 4               # (never seen: a dozen numbers) -> marker here, the object by itself below
                host[:4] = numpy.array([0xffffffff if big else len(blob)], dtype="<u4").view(numpy.uint8)
                if not big:
                    host[4:4 + len(blob)] = numpy.frombuffer(blob, dtype=numpy.uint8)
                wire.copy_(torch.from_numpy(host))
                dist.broadcast(wire, 0)
                if big:
                    tdist.broadcast_object(library, 0)
            else:
                work = dist.broadcast(wire, 0, async_op=True)
                held = 0
                if overlap:
                    held = bamio.preingest(args.bam, (rank, world), 50, stop=work.is_completed,
                                           chunk=int(os.environ.get("TIDDIT_INGEST_CHUNK", str(448 << 20))),
                                           **({} if track is None else {"track_bin_size": track[0]}))
                work.wait()
                host = wire.cpu().numpy()
                size = int(host[:4].view("<u4")[0])
                library = tdist.broadcast_object(None, 0) if size == 0xffffffff else pickle.loads(host[4:4 + size].tobytes())
                STAGE_NOTES["batches ingested beside rank 0's statistics"] = held
    max_ins_len = args.i if args.i else library["percentile_insert_size"]
    T["library statistics"] = time.time() - t
    genotype_job = None
    if sites_path is not None:
        # TIDDIT_GENOTYPE: the sites are read now (their windows need max_ins_len) — a bad file ends the job before the scan
        from . import tiddit_genotype
        t = time.time()
        try:
            meta, records = tiddit_genotype.parse_vcf(sites_path)
            sites, rules = tiddit_genotype.sites_of(records, contig_number, contig_length, max_ins_len)
        except tiddit_genotype.SitesError as e:
            if gc_job is not None and "thread" in gc_job:
                gc_job["thread"].join()                      # (no helper thread outlives the error)
            from . import bamio
            bamio.set_carry(None)                            # (nor the batches and the reader the statistics kept for the scan)
            print("error, TIDDIT_GENOTYPE={}: {}".format(sites_path, e))
            sys.exit(1)
        genotype_job = {"path": sites_path, "meta": meta, "records": records, "sites": sites, "rules": rules, "sites (host)": time.time() - t,
                        "depth": genotype_depth}
    if gc_job is not None and gc_mode != "after":
        start_gc()              # (the N-rank job and TIDDIT_GC_OVERLAP=scan: beside the scan only)

    t = time.time()
    # one process: the blocks of discordants / splits / clips are placed by a thread while the job goes on (tiddit_cluster takes the tables
    # over, not the files); finish_writes() below waits for it.  TIDDIT_BACKGROUND_WRITES=0: written before tiddit_signal.main returns.
    tiddit_signal.BACKGROUND_WRITES = (not multi) and os.environ.get("TIDDIT_BACKGROUND_WRITES", "1") != "0"
    # TIDDIT_VARIANTS=1: the scan also packs every placed record into the evidence store the native variant stage reads (on N ranks:
    # every rank the records of its own shard)
    # TIDDIT_GENOTYPE needs the same store, with or without the variant stage
    # ... and so do TIDDIT_DEPTH_DIST and TIDDIT_CLIPS_VCF
    tiddit_signal.KEEP_EVIDENCE = os.environ.get("TIDDIT_VARIANTS") == "1" or genotype_job is not None or depth_dist or clips_vcf is not None
    if track is not None:
        # TIDDIT_COV_TRACK: the scan fills a second histogram — every contig, the track's bin size and mapq cut — from the same batches
        tiddit_signal.COV_TRACK = (track[0], track[1])
    if allele_sites is not None:
        # TIDDIT_ALLELES: ... and counts the reads' bases at the sites, one launch per batch
        tiddit_signal.ALLELES = (allele_sites.site_pos, allele_sites.site_off, alleles[1])
        if phase is not None:
            # TIDDIT_PHASE: ... and stores a key per (read, phaseable site it shows REF or ALT at), one more launch per batch inside that push
            # (the indel counter's capacity rule; more than 2^31 - 1 sites are refused here, before the scan)
            try:
                tiddit_signal.ALLELES += ((tiddit_phase.site_codes(allele_sites), min(max(os.path.getsize(args.bam) // 16, 1 << 16), 1 << 26), 64) + phase,)
            except ValueError as e:
                print("error, TIDDIT_PHASE={}: {}".format(os.environ.get("TIDDIT_PHASE"), e))
                sys.exit(1)
    if qc:
        # TIDDIT_QC: ... and fills the read-level QC tables, two launches per batch
        tiddit_signal.QC = True
    if dups:
        # TIDDIT_DUPS: ... and stores a duplicate key per fragment and pair, one launch per batch
        tiddit_signal.DUPS = True
    if indels is not None:
        # TIDDIT_INDELS: ... and a key per small indel of the reads' CIGARs, one launch per batch
        tiddit_signal.INDELS = indels
    if indels_norm or snvs is not None or small_vcf is not None or clips_align is not None or clips_far is not None:
        # TIDDIT_INDELS_NORM / TIDDIT_SNVS / TIDDIT_SMALL_VCF / TIDDIT_CLIPS_ALIGN / TIDDIT_CLIPS_FAR: the reference goes into HBM before the scan (every
        # contig of the BAM header: read, uploaded, packed to 4-bit codes), ONCE: the indel kernel moves every event as far left as it allows, the SNV
        # kernel compares every aligned base with it, the small-variant VCF takes its deletion records' bases from it, the clip stage searches it for
        # the sites' consensus, and all hold the same handle
        t_ref = time.time()
        reference, t_read, t_load = refseq.load_for_bam(norm_fasta, chromosomes, [contig_length[c] for c in chromosomes])
        T["reference into HBM (%s)" % " + ".join(k for k, on in (("TIDDIT_INDELS_NORM", indels_norm), ("TIDDIT_SNVS", snvs is not None),
                                                                  ("TIDDIT_SMALL_VCF", small_vcf is not None),
                                                                  ("TIDDIT_CLIPS_ALIGN", clips_align is not None),
                                                                  ("TIDDIT_CLIPS_FAR", clips_far is not None)) if on)] = time.time() - t_ref
        T["  reference: file read (host)"] = t_read
        T["  reference: upload + ref_pack (returns when packed)"] = t_load
        if indels_norm:
            tiddit_signal.INDEL_REFERENCE = reference
        if snvs is not None:
            # TIDDIT_SNVS: ... and a key per base that differs from the reference, one launch per batch
            tiddit_signal.SNVS = snvs
            tiddit_signal.SNV_REFERENCE = reference
        if small_vcf is not None:
            # TIDDIT_SMALL_VCF: ... and +1 / -1 at the ends of every eligible read's aligned spans, one launch per batch: one more element
            # in ONE partner's setting, whose counter carries the handle back
            if snvs is not None:
                tiddit_signal.SNVS = snvs + ("depth",)
            else:
                tiddit_signal.INDELS = indels + ("depth",)
    if clips is not None:
        # TIDDIT_CLIPS: ... and a key per soft clip of the reads, one launch per batch
        tiddit_signal.CLIPS = clips
        # TIDDIT_CLIPS_INS: ... and a key per further chunk of 28 clipped bases, one more launch per batch
        tiddit_signal.CLIPS_INS = clips_ins is not None
    if str_loci is not None:
        # TIDDIT_STR: ... and a key per (read, known repeat locus in its reach), one launch per batch
        str_tap = tiddit_str.attach(str_loci, strs[1:])
        T["str loci ({} accepted; host)".format(len(str_loci))] = t_loci
    with stage("tiddit: signal extraction + coverage"):
        signal_main = tiddit_signal.main_sharded if multi else tiddit_signal.main
        try:
            coverage_data = signal_main(args.bam, args.ref, prefix, min_mapq, max_ins_len, sample_id, args.threads, args.min_contig,
                                        False, args.min_anchor_len, args.min_clip_len)
        finally:
            if gc_job is not None and gc_mode == "after":
                tiddit_signal.AFTER_SCAN.remove(start_gc)
            tiddit_signal.BACKGROUND_WRITES = False
            tiddit_signal.KEEP_EVIDENCE = False
            if track is not None:
                tiddit_signal.COV_TRACK = None
            tiddit_signal.ALLELES = None
            tiddit_signal.QC = None
            tiddit_signal.DUPS = None
            tiddit_signal.INDELS = None
            tiddit_signal.INDEL_REFERENCE = None      # (the counter holds it from here on)
            tiddit_signal.SNVS = None
            tiddit_signal.SNV_REFERENCE = None        # (the same)
            tiddit_signal.CLIPS = None
            tiddit_signal.CLIPS_INS = False
            tiddit_str.detach()
            if gc_job is not None and sys.exc_info()[0] is not None and "thread" in gc_job:
                gc_job["thread"].join()          # (the scan failed: no helper thread outlives the error)
    if rank == 0:
        print("extracted signals in:")
        print(t - time.time())
    T["signal extraction + coverage"] = time.time() - t
    T.update({"  " + k: v for k, v in tiddit_signal.STAGE_SECONDS.items()})
    if track is not None:
        bins, tiddit_signal.COV_TRACK_BINS = tiddit_signal.COV_TRACK_BINS, None
        if rank == 0:
            # what run_cov writes for `--cov -z Z -q Q [-w] -o {o}`, through the same function
            from . import tiddit_coverage
            t = time.time()
            tiddit_coverage.print_coverage(bins, bam_header, track[0], track[2], "{}.{}".format(prefix, track[2]))
            T["coverage track ({o}.bed / {o}.wig, from the scan's second histogram)"] = time.time() - t
        del bins
    if allele_sites is not None:
        counter, tiddit_signal.ALLELE_COUNTER = tiddit_signal.ALLELE_COUNTER, None
        t = time.time()
        allele_table = tiddit_alleles.main(counter, allele_sites, prefix, multi=multi, rank=rank)
        T["allele counts ({o}.alleles.tab)"] = time.time() - t
        T.update({"  " + k: v for k, v in tiddit_alleles.STAGE_SECONDS.items()})
        if phase is not None:
            # TIDDIT_PHASE: the finish of the observation store the counter carries, the two files, one summary line
            t = time.time()
            tiddit_phase.main(counter, allele_sites, allele_table, prefix, names=chromosomes)
            T["phase sets ({o}.phase.tab, {o}.phase.blocks.tab)"] = time.time() - t
            T.update({"  " + k: v for k, v in tiddit_phase.STAGE_SECONDS.items()})
            STAGE_NOTES.update(tiddit_phase.STAGE_NOTES)
    if qc:
        counter, tiddit_signal.QC_COUNTER = tiddit_signal.QC_COUNTER, None
        t = time.time()
        tiddit_qc.main(counter, prefix, multi=multi, rank=rank)
        T["qc tables ({o}.qc.tab)"] = time.time() - t
        T.update({"  " + k: v for k, v in tiddit_qc.STAGE_SECONDS.items()})
    if dups:
        counter, tiddit_signal.DUP_COUNTER = tiddit_signal.DUP_COUNTER, None
        t = time.time()
        tiddit_dup.main(counter, prefix)
        T["duplicates ({o}.dup.tab)"] = time.time() - t
        T.update({"  " + k: v for k, v in tiddit_dup.STAGE_SECONDS.items()})
    if indels is not None:
        # (behind the scan: coverage_data is final, no later stage writes into it)
        counter, tiddit_signal.INDEL_COUNTER = tiddit_signal.INDEL_COUNTER, None
        pile = counter.depth                          # (TIDDIT_SMALL_VCF without TIDDIT_SNVS: the depth handle, else None)
        t = time.time()
        indel_kept = {} if small_vcf is not None else None
        tiddit_indels.main(counter, prefix, coverage_data, chromosomes, indels[0], keep=indel_kept)
        T["small indels ({o}.indels.tab)"] = time.time() - t
        T.update({"  " + k: v for k, v in tiddit_indels.STAGE_SECONDS.items()})
        STAGE_NOTES.update(tiddit_indels.STAGE_NOTES)
    if str_loci is not None:
        # (the same: the sort, the genotype rule and the file)
        counter, str_tap.counter = str_tap.counter, None
        t = time.time()
        tiddit_str.main(counter, str_loci, prefix, strs[1:])
        T["tandem repeats ({o}.str.tab)"] = time.time() - t
        T.update({"  " + k: v for k, v in tiddit_str.STAGE_SECONDS.items()})
        STAGE_NOTES.update(tiddit_str.STAGE_NOTES)
    if snvs is not None:
        # (the same)
        counter, tiddit_signal.SNV_COUNTER = tiddit_signal.SNV_COUNTER, None
        pile = counter.depth                          # (TIDDIT_SMALL_VCF: the depth handle, else None)
        t = time.time()
        snv_kept = {} if small_vcf is not None else None
        tiddit_snvs.main(counter, prefix, coverage_data, chromosomes, snvs[0], keep=snv_kept)
        T["snv candidates ({o}.snvs.tab)"] = time.time() - t
        T.update({"  " + k: v for k, v in tiddit_snvs.STAGE_SECONDS.items()})
        STAGE_NOTES.update(tiddit_snvs.STAGE_NOTES)
    if small_vcf is not None:
        # TIDDIT_SMALL_VCF: behind the two stages whose finished rows it genotypes — the prefix sum over the difference array the scan
        # left, one gather launch per table, the records' text
        t = time.time()
        tiddit_small_vcf.main(pile, prefix, chromosomes, tiddit_clip_vcf.header_parts(bam_header, sample_id, version),
                              snv_kept["rows"] if snvs is not None else None, indel_kept["rows"] if indels is not None else None, reference, indels_norm)
        T["small variants ({o}.small.vcf)"] = time.time() - t
        T.update({"  " + k: v for k, v in tiddit_small_vcf.STAGE_SECONDS.items()})
        STAGE_NOTES.update(tiddit_small_vcf.STAGE_NOTES)
    if clips is not None:
        # (the same)
        counter, tiddit_signal.CLIP_COUNTER = tiddit_signal.CLIP_COUNTER, None
        t = time.time()
        clip_stage_rows = None if clips_vcf is None else {}
        try:
            # TIDDIT_CLIPS_ALIGN: ... and the sites' consensus is searched in the reference, behind the finish, where the rows lie
            # TIDDIT_CLIPS_FAR: ... and placed genome-wide by its seed, the same way
            # TIDDIT_CLIPS_INS: ... and the rows are extended from the second store, paired and closed, the same way
            tiddit_clips.main(counter, prefix, coverage_data, chromosomes, clips[0], None if clips_align is None else (reference,) + clips_align,
                              far=None if clips_far is None else (reference,) + clips_far, ins=clips_ins, keep=clip_stage_rows, mei=clips_mei)
        finally:
            if (clips_align is not None or clips_far is not None) and not indels_norm and snvs is None:
                reference.close()                     # (only these switches loaded it)
        T["clip sites ({o}.clips.tab)"] = time.time() - t
        T.update({"  " + k: v for k, v in tiddit_clips.STAGE_SECONDS.items()})
        if clips_align is not None:
            T.update({"  " + k: v for k, v in tiddit_clip_align.STAGE_SECONDS.items()})
        if clips_far is not None:
            T.update({"  " + k: v for k, v in tiddit_clip_far.STAGE_SECONDS.items()})
        if clips_ins is not None:
            T.update({"  " + k: v for k, v in tiddit_clip_ins.STAGE_SECONDS.items()})
        if clips_mei is not None:
            T.update({"  " + k: v for k, v in tiddit_clip_mei.STAGE_SECONDS.items()})
        STAGE_NOTES.update(tiddit_clips.STAGE_NOTES)
        if clips_vcf is not None:
            # TIDDIT_CLIPS_VCF: the stages' rows become junctions, and one launch counts the reads that cross every breakpoint intact over
            # the store the scan left, which stays where it is for the stages below
            from . import tiddit_variant
            if tiddit_variant.LIVE_STORE is None:
                raise RuntimeError("TIDDIT_CLIPS_VCF: the scan left no evidence store")
            t = time.time()
            vcf_counts = tiddit_clip_vcf.main(tiddit_variant.LIVE_STORE, prefix, chromosomes, clips_vcf,
                                              tiddit_clip_vcf.header_parts(bam_header, sample_id, version),
                                              clip_stage_rows.get("align"), clip_stage_rows.get("far"), clip_stage_rows.get("ins"),
                                              mei=None if clips_mei is None else (clips_mei[1], clip_stage_rows.get("mei", []),
                                                                                  tiddit_clip_mei.library_index(clips_mei[0])[1]))
            print(tiddit_clip_vcf.summary_line(vcf_counts))
            T["clip junction vcf ({o}.clips.vcf)"] = time.time() - t
            T.update({"  " + k: v for k, v in tiddit_clip_vcf.STAGE_SECONDS.items()})
    try:
        _after_scan(args, prefix, rank, multi, T, gc_job, start_gc if gc_job is not None else None, chromosomes, contigs, contig_length, samples,
                    library, coverage_data, bam_header, max_ins_len, min_mapq, sample_id, version, contig_number, own_group if multi else False,
                    genotype_job, depth_dist, cnv, (allele_table, allele_sites) if ascn else None)
    except BaseException:
        # no helper thread outlives the error: the writer thread of BACKGROUND_WRITES is joined (its own error, if any, is not the one to report)
        try:
            tiddit_signal.finish_writes()
        except BaseException:
            pass
        raise
    finally:
        from . import tiddit_variant
        if tiddit_variant.LIVE_STORE is not None:                        # (a store the variant stage did not take: freed here)
            tiddit_variant.LIVE_STORE.close()
            tiddit_variant.LIVE_STORE = None


def _after_scan(args, prefix, rank, multi, T, gc_job, start_gc, chromosomes, contigs, contig_length, samples, library, coverage_data, bam_header,
                max_ins_len, min_mapq, sample_id, version, contig_number, own_group, genotype_job=None, depth_dist=False, cnv=None, ascn=None):
    """run_sv behind the BAM scan: GC bins, ploidy table, copy-number segments (TIDDIT_CNV), allele-specific ones (TIDDIT_ASCN; ascn: the
    counter table and the sites of TIDDIT_ALLELES), clustering, candidates table, the signal files complete, the depth
    distributions (TIDDIT_DEPTH_DIST=1), the variant stage (TIDDIT_VARIANTS=1), the genotypes of known sites (TIDDIT_GENOTYPE)"""
    from . import tiddit_cluster, tiddit_coverage_analysis, tiddit_gc, tiddit_signal
    from .trace import stage
    if multi:
        import torch.distributed as dist
        from . import dist as tdist
    t = time.time()
    gc_dictionary = None
    with stage("tiddit: GC bins"):
        if gc_job is None:
            if rank == 0:
                gc_dictionary = tiddit_gc.main(args.ref, chromosomes, args.threads, 50, 0.5)
        else:
            start_gc()                          # (already running unless the thread waits for the end of the scan, or the scan never got there)
            gc_job["thread"].join()
            if "error" in gc_job:
                raise gc_job["error"]
            gc_dictionary = gc_job["result"]
            if multi:                           # every rank's contigs to rank 0 (int8 bins: 60 MB for a human genome)
                import pickle
                parts = tdist.gather_bytes(pickle.dumps(gc_dictionary, protocol=4), 0)
                if rank == 0:
                    merged = {}
                    for p_ in parts:
                        merged.update(pickle.loads(p_))
                    gc_dictionary = {c: merged[c] for c in chromosomes}
    T["GC bins"] = time.time() - t
    if gc_job is not None:
        T["  GC bins, on their own thread beside the scan"] = gc_job["seconds"]
    if rank == 0:
        t = time.time()
        with stage("tiddit: ploidy"):
            library = tiddit_coverage_analysis.determine_ploidy(coverage_data, contigs, library, args.n, prefix, args.c, args.ref, 50,
                                                                bam_header, gc_dictionary)
        print("calculated coverage in:")
        print(time.time() - t)
        T["ploidy (masked medians)"] = time.time() - t
        if cnv is not None:
            # TIDDIT_CNV: rank 0 holds the (reduced) coverage bins, every contig's GC bins and the ploidy table from here on
            from . import tiddit_cnv
            t = time.time()
            with stage("tiddit: copy-number segments"):
                if ascn is None:
                    tiddit_cnv.main(coverage_data, gc_dictionary, library, contigs, contig_length, args.min_contig, cnv, prefix)
                else:
                    # (the same two halves, the bins kept: x stays on the device for the stage below)
                    cnv_bins = tiddit_cnv.bins_stage(coverage_data, gc_dictionary, library, contigs, contig_length, args.min_contig, cnv)
                    tiddit_cnv.segments_stage(cnv_bins, contig_length, prefix)
            T["copy-number segments ({o}.cnv.bed)"] = time.time() - t
            T.update({"  " + k: v for k, v in tiddit_cnv.STAGE_SECONDS.items()})
            if ascn is not None:
                # TIDDIT_ASCN: ... and the counter table of TIDDIT_ALLELES (on N ranks the sum of every rank's)
                from . import tiddit_ascn
                t = time.time()
                with stage("tiddit: allele-specific copy number"):
                    tiddit_ascn.main(cnv_bins, ascn[0], ascn[1], contig_number, contig_length, prefix)
                del cnv_bins
                T["allele-specific copy number ({o}.ascn.bed)"] = time.time() - t
                T.update({"  " + k: v for k, v in tiddit_ascn.STAGE_SECONDS.items()})
    if not args.e:
        args.e = int(library["avg_insert_size"] / 2.0)
    if not args.e:
        args.e = 50
    t = time.time()
    with stage("tiddit: clustering"):
        cluster_main = tiddit_cluster.main_sharded if multi else tiddit_cluster.main
        sv_clusters = cluster_main(prefix, contigs, contig_length, samples, library["mp"], args.e, args.l, max_ins_len, args.min_contig,
                                   args.skip_assembly, args.r)
    T["clustering"] = time.time() - t
    T.update({"  " + k: v for k, v in tiddit_cluster.STAGE_SECONDS.items()})
    if rank == 0:
        print("generated clusters in")
        print(T["clustering"])
        t = time.time()
        write_candidates(prefix + ".candidates.tab", contigs, sv_clusters)
        T["candidates table"] = time.time() - t
    tiddit_signal.finish_writes()                                        # the signal files are complete from here on
    if tiddit_signal.WRITE_SECONDS:
        T["signal files placed (writer thread, beside ploidy and clustering)"] = tiddit_signal.WRITE_SECONDS["writer thread"]
        T["  waited for the writer thread"] = tiddit_signal.WRITE_SECONDS["waited for it"]
    if depth_dist:
        # TIDDIT_DEPTH_DIST: one launch over the store the scan left, which stays where it is for the stages below (a store nobody
        # takes afterwards is freed by run_sv)
        from . import tiddit_depth_dist, tiddit_variant
        if tiddit_variant.LIVE_STORE is None:
            raise RuntimeError("TIDDIT_DEPTH_DIST: the scan left no evidence store")
        t = time.time()
        with stage("tiddit: depth distribution"):
            tiddit_depth_dist.main(tiddit_variant.LIVE_STORE, prefix, chromosomes, [contig_length[c] for c in chromosomes])
        T["depth distribution ({o}.depth_dist.tab, {o}.depth_summary.tab)"] = time.time() - t
        T.update({"  " + k: v for k, v in tiddit_depth_dist.STAGE_SECONDS.items()})
    if os.environ.get("TIDDIT_VARIANTS") == "1":
        # the native variant stage (tiddit_variant.py over the evidence store the scan filled, tiddit_vcf_header.py): {prefix}.vcf.  On N
        # ranks every rank takes part (the counts over its shard's store); rank 0 types the variants and writes the file.
        from . import tiddit_variant, tiddit_vcf_header
        t = time.time()
        tiddit_variant.KEEP_STORE = genotype_job is not None         # (the store serves the genotyping behind this stage, which frees it)
        try:
            with stage("tiddit: variant typing"):
                variant_stage(tiddit_variant, tiddit_vcf_header, prefix, contigs, bam_header, library, sample_id, version, args, sv_clusters,
                              min_mapq, samples, coverage_data, contig_number, max_ins_len, gc_dictionary,
                              entry=tiddit_variant.main_sharded if multi else tiddit_variant.main)
        finally:
            tiddit_variant.KEEP_STORE = False
        T["variant typing (native)"] = time.time() - t
        T.update({"  " + k: v for k, v in tiddit_variant.STAGE_SECONDS.items()})
        if rank == 0:
            print("analyzed clusters in")
            print(T["variant typing (native)"])
    elif rank == 0 and genotype_job is not None:
        pass                                                             # (TIDDIT_GENOTYPE alone: no {prefix}.vcf, the genotypes below)
    elif rank == 0:
        # Without TIDDIT_VARIANTS=1 the run stops at the candidates table.  When the reference package itself is importable (it needs
        # pysam) the candidates are handed to it, as the reference's driver does (__main__.py:193-207), so that a full installation
        # still ends with {prefix}.vcf.
        try:
            import tiddit.tiddit_variant as tiddit_variant
            import tiddit.tiddit_vcf_header as tiddit_vcf_header
        except Exception:
            tiddit_variant = tiddit_vcf_header = None
        t = time.time()
        if variant_stage(tiddit_variant, tiddit_vcf_header, prefix, contigs, bam_header, library, sample_id, version, args, sv_clusters, min_mapq,
                         samples, coverage_data, contig_number, max_ins_len, gc_dictionary):
            T["variant typing (reference package)"] = time.time() - t
        else:
            print("variant typing/filtering (tiddit_variant) is outside this build's scope; candidates written to {}.candidates.tab "
                  "(TIDDIT_VARIANTS=1 runs the native variant stage)".format(prefix))
    if genotype_job is not None:
        t = time.time()
        with stage("tiddit: genotyping of known sites"):
            genotype_stage(genotype_job, args, prefix, samples, library, coverage_data, bam_header, gc_dictionary, min_mapq, max_ins_len, sample_id,
                           version, contig_number, T)
        T["genotyping of known sites ({o}.genotyped.vcf)"] = time.time() - t
    if multi:
        dist.barrier()                                                   # every output file exists when any rank returns
        if own_group:
            # (a process that exits with its RCCL group alive can die in the group's watchdog thread while the HIP runtime unloads)
            dist.destroy_process_group()


def genotype_stage(job, args, prefix, samples, library, coverage_data, bam_header, gc_dictionary, min_mapq, max_ins_len, sample_id, version,
                   contig_number, T):
    """TIDDIT_GENOTYPE: {prefix}.genotyped.vcf from the evidence store the scan left (after the variant stage, if that ran) and the
    cluster table of the job's signal tables on the device (tiddit_genotype.py); both are freed here"""
    from . import tiddit_genotype, tiddit_region, tiddit_signal, tiddit_variant, tiddit_vcf_header
    T["  sites (host, before the scan)"] = job["sites (host)"]
    t = time.time()
    tables = tiddit_signal.written_tables("{}_tiddit/discordants_{}.tab".format(prefix, samples[0]), "{}_tiddit/splits_{}.tab".format(prefix, samples[0]))
    if tables is None:
        raise RuntimeError("TIDDIT_GENOTYPE: the signal tables of this job are gone (its .tab files changed under it)")
    store = tiddit_variant.take_store(args.bam, min_mapq, int(max_ins_len))
    links = None
    try:
        if store is None:
            store = tiddit_region.build_store(args.bam, min_mapq, int(max_ins_len))
            T["  evidence store (one ingest pass)"] = time.time() - t
            t = time.time()
        links = tiddit_genotype.links_of_tables(tables, library["mp"], args.min_contig)
        T["  links handle (cluster table, upload + sort)"] = time.time() - t
        columns = tiddit_genotype.genotype_sites(store, links, job["sites"], args, library, coverage_data, gc_dictionary, min_mapq, max_ins_len,
                                                 contig_number=contig_number, rules=job["rules"], depth=job["depth"])
    finally:
        if links is not None:
            links.close()
        if store is not None:
            store.close()
    T.update({"  " + k: v for k, v in tiddit_genotype.STAGE_SECONDS.items()})
    t = time.time()
    head = tiddit_genotype.header(tiddit_vcf_header.main(bam_header, library, sample_id, version), job["meta"], job["path"], max_ins_len,
                                  depth=job["depth"])
    tiddit_genotype.write_vcf(prefix + ".genotyped.vcf", head, job["records"], columns, depth=job["depth"])
    T["  header + file"] = time.time() - t
    missed = job["rules"].count("missed")
    STAGE_NOTES["sites genotyped"] = len(columns)
    STAGE_NOTES["sites whose breakpoints fit their REGIONA/REGIONB in neither order (window rule)"] = missed
    print("genotyped {} sites of {} into {}.genotyped.vcf".format(len(columns), job["path"], prefix))
    if missed:
        print("note: {} of them have breakpoints outside their REGIONA/REGIONB and took the window rule".format(missed))


def main(argv=None):
    version = "3.9.5"
    if argv is not None:
        sys.argv = [sys.argv[0]] + list(argv)
    parser = argparse.ArgumentParser("""tiddit-{}""".format(version), add_help=False)
    parser.add_argument("--sv", help="call structural variation", required=False, action="store_true")
    parser.add_argument("--cov", help="generate a coverage bed file", required=False, action="store_true")
    args, unknown = parser.parse_known_args()
    if args.sv:
        from .hostutil import quiet_gc
        # The job's helper threads (row building, GC bins) spend their time inside the library without the GIL and need it only for
        # moments in between; with CPython's default 5 ms switch interval each of those moments waits up to 5 ms while the main thread
        # runs a Python loop (the GC thread beside merge + write: 1.35 s for 0.46 s of work on a 3-Gb genome).
        interval = sys.getswitchinterval()
        sys.setswitchinterval(min(interval, 0.0005))
        try:
            with quiet_gc(freeze=True):      # one job, one process: the collector stays off from the first stage to the last
                run_sv(_sv_parser().parse_args(), version)
        finally:
            sys.setswitchinterval(interval)
    elif args.cov:
        run_cov(_cov_parser().parse_args())
    else:
        parser.print_help()


if __name__ == "__main__":
    main()
