"""The VCF header of ``tiddit --sv`` (tiddit_vcf_header.py:4-68 of the reference), same signature and the same text.

``main(bam_header, library, sample_id, version)`` -> the header lines joined by newlines (no trailing newline), including the
``##TIDDITcmd`` line built from ``sys.argv`` at the time of the call.
"""
import sys

_ALT = (("DEL", "Deletion"), ("DUP", "Duplication"), ("DUP:TANDEM", "Tandem duplication"), ("DUP:INV", "Inverted tandem duplication"),
        ("INV", "Inversion"), ("INS", "Insertion"), ("BND", "Break end"))

_INFO = (("SVTYPE", "1", "String", "Type of structural variant"),
         ("END", "1", "Integer", "End of an intra-chromosomal variant"),
         ("SVLEN", ".", "Integer", "Difference in length between REF and ALT alleles"),
         ("LFA", "2", "Integer", "Read-pairs and split reads in region A"),
         ("LFB", "2", "Integer", "Read-pairs and split reads in region B"),
         ("LTE", "2", "Integer", "Read-pairs and split reads supporting the event"),
         ("CTG", "1", "String", "Sequence of contig"),
         ("REGIONA", "2", "Integer", "Start and end of regionB"),       # (sic: the reference's description of REGIONA)
         ("REGIONB", "2", "Integer", "Start and end of regionB"))

_FILTER = (("BelowExpectedLinks", "The number of links or reads between A and B is too small"),
           ("FewLinks", "Unexpectedly low fraction of discordant reads betwen A and B"),
           ("UnexpectedCoverage", "The coverage of the window on chromosome B or A is higher than 4*average coverage"),
           ("Smear", "Window A and Window B overlap"),
           ("RegionalQ", "The mapping quality of the region is lower than the user set limit"),
           ("MinSize", "The variant is smaller than the user set limit"),
           ("Ploidy", "Intrachromosomal variant on a chromosome having 0 ploidy"),
           ("SplitsVSDiscs", "large variant supported mainly by split reads (and not discorant pairs) "),
           ("Density", "The discordant reads cluster too tightly"))

_FORMAT = (("GT", "1", "String", "Genotype"),
           ("CN", "1", "Integer", "Copy number genotype for imprecise events"),
           ("DV", "1", "Integer", "Number of paired-ends that support the event"),
           ("RV", "1", "Integer", "Number of split reads that support the event"),
           ("DR", "2", "Integer", "Number of paired-ends that supporting the reference allele (breakpoint A, and B)"),
           ("RR", "2", "Integer", "Number of reads supporting the reference allele (breakpoint A, and B)"),
           ("COV", "3", "Float", "Coverage (at A,B, and between)"),
           ("LQ", "2", "Float", "Fraction of low quality reads"))


def cmd_line():
    """the ``##TIDDITcmd`` line: the process's command line as it stands now"""
    return '##TIDDITcmd="' + " ".join(sys.argv) + '"'


def contig_lines(bam_header):
    """the ``##contig`` lines, one per ``@SQ`` of the BAM header"""
    return ["##contig=<ID={},length={}>".format(c["SN"], c["LN"]) for c in bam_header["SQ"]]


def column_line(sample_id):
    return "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + sample_id


def main(bam_header, library, sample_id, version):
    lines = ["##fileformat=VCFv4.1", "##source=TIDDIT-" + version]
    lines += ['##ALT=<ID={},Description="{}">'.format(i, d) for i, d in _ALT]
    lines += contig_lines(bam_header)
    lines += ['##INFO=<ID={},Number={},Type={},Description="{}">'.format(*row) for row in _INFO]
    lines += ['##FILTER=<ID={},Description="{}">'.format(*row) for row in _FILTER]
    lines += ['##FORMAT=<ID={},Number={},Type={},Description="{}">'.format(*row) for row in _FORMAT]
    lines.append("##LibraryStats=TIDDIT-{} Coverage={}  ReadLength={} MeanInsertSize={} STDInsertSize={} Reverse_Forward={}".format(
        version, library["avg_coverage"], library["avg_read_length"], library["avg_insert_size"], library["std_insert_size"], library["mp"]))
    lines.append(cmd_line())
    lines.append(column_line(sample_id))
    return "\n".join(lines)
