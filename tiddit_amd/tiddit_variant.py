"""Variant typing, filtering, genotyping and scoring of the SV candidates — tiddit_variant.pyx of the reference, with its
signature: ``main(bam_file_name, sv_clusters, args, library, min_mapq, samples, coverage_data, contig_number, max_ins_len, gc)``
returns the reference's ``variants`` dict ({contig: [[pos, vcf fields], ...]}).

The evidence comes from the device, all candidates at once:
  1. the three coverage means of every candidate in one call (tiddit_region.candidate_means, :265-283, :307-315);
  2. the host pre-filters of define_variant (:251-284) pick the candidates that need regional counts;
  3. ONE tdt_region_counts_packed launch answers every get_region call of those candidates (:290-305) from the evidence store —
     the packed records the signal scan of this process left in HBM, or, when there is none (the module swapped into another
     driver), a store built by one device-ingest pass over the file.  On N ranks (:func:`main_sharded`) every rank holds the store
     of its shard of the file, answers all of rank 0's queries in one launch, and the partial counts are summed on rank 0.
The typing layer (:define_variant, :finish) takes that evidence as arguments — the get_region results keyed by
(chrom, start, end, bp) and the means per candidate — and keeps every visible quirk of the reference's output.
"""
import math

import numpy

from . import tiddit_region

PERCENTILES = [1, 5, 10, 20, 30, 40, 50, 60, 70, 75, 80, 85, 90, 95, 97.5, 99]
FORMAT_COL = "GT:CN:COV:DV:RV:LQ:RR:DR"


def percentile(a, q):
    """nearest-rank percentiles of a (0 for every q when a is empty) (:9-21)"""
    s = sorted(a)
    return [s[int(math.ceil((len(s) * v) / 100.0)) - 1] if len(s) else 0 for v in q]


def scoring(d, percentiles):
    """QUAL: 50 for contig support, 5 per percentile the pair / split ratios reach at either breakpoint; the best of those (:24-52)"""
    score = [0]
    if d["n_contigs"]:
        score.append(50)
    for n, keys in (("n_discordants", (("FA", "refFA"), ("FB", "refFB"))), ("n_splits", (("RA", "refRA"), ("RB", "refRB")))):
        if d[n]:
            for pkey, ref in keys:
                ratio = d[n] / (d[ref] + d[n])
                score.append(sum(5 for p in percentiles[pkey] if ratio >= p))
    return max(score)


def region_tuple(counts, start, end):
    """int64[7] of the kernel -> get_region's return value (:141-151): coverage is a float, frac_low_q the int 0 without reads"""
    bases, n_reads, low_q, n_discs, n_splits, crossing_f, crossing_r = (int(x) for x in counts)
    coverage = bases / (end - start + 1)
    frac_low_q = low_q / float(n_reads) if n_reads > 0 else 0
    return (coverage, frac_low_q, n_discs, n_splits, crossing_f, crossing_r)


def copy_number(chrA, covM, args, library):
    """the CN of an intrachromosomal variant (:159-165): the coverage between the breakpoints in units of one copy of chrA"""
    avg = library["avg_coverage_{}".format(chrA)]
    if avg != 0:
        return int(round(covM * library["contig_ploidy_{}".format(chrA)] / avg))
    return int(round(covM * args.n / library["avg_coverage"]))


def find_sv_type(chrA, chrB, inverted, non_inverted, args, sample_data, samples, library):
    """(:153-189) -> (svtype, copy number); the copy number is the last sample's"""
    if chrA != chrB:
        return "BND", "."
    p = library["contig_ploidy_{}".format(chrA)]
    avg = library["avg_coverage_{}".format(chrA)]
    for sample in samples:
        cn = copy_number(chrA, sample_data[sample]["covM"], args, library)
    if p > args.n * 10:                        # mitochondria or similar
        if cn > p * 1.05:
            return ("DUP:INV" if inverted else "DUP:TANDEM"), cn
        if cn < p * 0.95:
            return "DEL", cn
        return ("INV" if inverted > non_inverted else "BND"), cn
    if cn > p:
        return ("DUP:INV" if inverted else "DUP:TANDEM"), cn
    if inverted > non_inverted:
        return "INV", cn
    if cn < p:
        return "DEL", cn
    return "BND", cn


def sv_filter(sample_data, args, chrA, chrB, posA, posB, max_ins_len, n_discordants, n_splits, library, n_discs_regionA, n_discs_regionB,
              n_splits_regionA, n_splits_regionB, n_contigs):
    """the FILTER column (:192-236)"""
    for sample in sample_data:
        sd = sample_data[sample]
        cap_a = args.max_coverage * library["avg_coverage_{}".format(chrA)]
        cap_b = args.max_coverage * library["avg_coverage_{}".format(chrB)]
        if sd["covA"] > cap_a or sd["covB"] > cap_b or sd["covM"] > cap_b:
            return "UnexpectedCoverage"
        if not n_contigs:
            few_pairs_ref = n_discordants < args.p_ratio * sd["refFA"] or n_discordants < args.p_ratio * sd["refFB"]
            few_splits_ref = n_splits < args.r_ratio * sd["refRA"] or n_splits < args.r_ratio * sd["refRB"]
            if few_pairs_ref and few_splits_ref:
                return "BelowExpectedLinks"
            few_pairs_cov = n_discordants < args.p_ratio * sd["covA"] or n_discordants < args.p_ratio * sd["covB"]
            few_splits_cov = n_splits < args.r_ratio * sd["covA"] or n_splits < args.r_ratio * sd["covB"]
            if few_pairs_cov and few_splits_cov:
                return "BelowExpectedLinks"
            if n_discordants > n_splits:
                if n_discordants < 0.25 * n_discs_regionA or n_discordants < 0.25 * n_discs_regionB:
                    return "FewLinks"
            elif n_splits < 0.25 * n_splits_regionA or n_splits < 0.25 * n_splits_regionB:
                return "FewLinks"
            if sd["QA"] > 0.2 or sd["QB"] > 0.2:
                return "RegionalQ"
            if n_discordants == 0 and chrA != chrB:
                return "SplitsVSDiscs"
        if n_contigs and chrA != chrB:
            if n_discordants < args.p:
                return "BelowExpectedLinks"
        elif n_contigs and (chrA == chrB and max_ins_len * 3 < abs(posB - posA)):
            if n_discordants < args.p:
                return "BelowExpectedLinks"
    return "PASS"


def survivors(chrA, sv_clusters, args, library, means):
    """the candidates of chrA that pass the host pre-filters of define_variant (:251-284), in the reference's order:
    -> [(chrB, cluster id, candidate, posA, posB, avg_a, avg_b)]"""
    out = []
    for chrB in sv_clusters[chrA]:
        for cid, c in sv_clusters[chrA][chrB].items():
            n_discordants, n_splits, n_contigs = c["N_discordants"], c["N_splits"], c["N_contigs"]
            if (n_discordants < args.p and n_splits < args.r) and not n_contigs:
                continue
            posA, posB = c["posA"], c["posB"]
            if chrA == chrB and posA > posB:
                posA, posB = posB, posA
            if chrA == chrB and abs(posA - posB) < args.z:
                continue
            m = means[(chrA, chrB, cid)]
            avg_a, avg_b = m["avg_a"], m["avg_b"]          # numpy.float64: a zero mean divides to inf / nan, as in the reference
            if avg_a > args.max_coverage * library["avg_coverage_{}".format(chrA)]:
                continue
            if (args.max_coverage * n_discordants / avg_a < args.p_ratio / 2 and args.max_coverage * n_splits / avg_a < args.r_ratio / 2) and not n_contigs:
                continue
            if avg_b == 0:
                continue
            if avg_b > args.max_coverage * library["avg_coverage_{}".format(chrB)]:
                continue
            if (args.max_coverage * n_discordants / avg_b < args.p_ratio / 2 and args.max_coverage * n_splits / avg_b < args.r_ratio / 2) and not n_contigs:
                continue
            out.append((chrB, cid, c, posA, posB, avg_a, avg_b))
    return out


def region_queries(chrA, chrB, c, posA, posB):
    """the get_region calls define_variant makes for one surviving candidate (:290-305), as (chrom, start, end, bp)"""
    q = [(chrA, c["startA"], c["endA"], posA), (chrB, c["startB"], c["endB"], posB)]
    if chrA == chrB and abs(posB - posA) < 1000:
        q.append((chrA, posA, posB, posA) if posA < posB else (chrA, posB, posA, posB))
    return q


def _genotype(c, sd, sample, args, n_contigs):
    """the GT every record of a candidate starts from (the three genotype blocks of define_variant)"""
    return genotype_of(len(c["sample_splits"][sample]), len(c["sample_discordants"][sample]), sd, args, n_contigs)


def genotype_of(n_sp, n_di, sd, args, n_contigs):
    """:func:`_genotype` from the sample's two support counts"""
    GT = "./."
    if n_sp >= args.r or n_di >= args.p:
        GT = "0/1"
    if sd["refRB"] < 0.1 * n_sp or sd["refRA"] < 0.1 * n_sp:
        GT = "1/1"
    if sd["refFB"] < 0.1 * n_di or sd["refFA"] < 0.1 * n_di:
        GT = "1/1"
    if n_contigs and (not n_di and not n_sp):
        if sd["covB"]:
            GT = "1/1" if sd["refRB"] / sd["covB"] < 0.2 else "0/1"
        else:
            GT = "1/1"
        if sd["covA"]:
            GT = "1/1" if sd["refRA"] / sd["covA"] < 0.2 else "0/1"
        else:
            GT = "1/1"
    return GT


def depth_genotype(GT, svtype, cn, ploidy):
    """the read-depth override of the GT of a <DEL> / <DUP...> record (the record loop of define_variant); GT itself otherwise"""
    if "DEL" in svtype:
        return "1/1" if cn == 0 else "0/1"
    if "DUP" in svtype:
        return "1/1" if cn >= 2 * ploidy else "0/1"
    return GT


def site_evidence(chrA, chrB, posA, posB, startA, endA, startB, endB, regions, cov_between):
    """one sample's evidence dict of a site (:290-315) from the get_region results; cov_between: covM of an intrachromosomal site
    whose breakpoints are 1000 bp or more apart (tiddit_region.candidate_means)"""
    covA, QA, discA, splitA, refFA, refRA = regions[(chrA, startA, endA, posA)]
    covB, QB, discB, splitB, refFB, refRB = regions[(chrB, startB, endB, posB)]
    sd = {"covA": covA, "QA": QA, "discA": discA, "splitA": splitA, "refRA": refRA, "refFA": refFA,
          "covB": covB, "QB": QB, "discB": discB, "splitB": splitB, "refRB": refRB, "refFB": refFB}
    if chrA != chrB:
        sd["covM"] = 0
    elif abs(posB - posA) < 1000:
        key = (chrA, posA, posB, posA) if posA < posB else (chrA, posB, posA, posB)
        sd["covM"] = regions[key][0]
    else:
        sd["covM"] = cov_between
    return sd


def _sample_column(GT, cn, sd, n_discordants, n_splits):
    return "{}:{}:{},{},{}:{}:{}:{},{}:{},{}:{},{}".format(GT, cn, sd["covA"], sd["covM"], sd["covB"], n_discordants, n_splits, sd["QA"], sd["QB"],
                                                          sd["refRA"], sd["refRB"], sd["refFA"], sd["refFB"])


def _ctg(c, n_contigs, contig_seqs):
    if not n_contigs:
        return "CTG=."
    for name in c["contigs"]:                   # (the last contig's sequence, as in the reference)
        if "_d_" in name:
            name = name.split("_d_")[0]
        ctgs = [contig_seqs[name]]
    return "CTG={}".format("|".join(ctgs))


def define_variant(chrA, sv_clusters, args, library, samples, max_ins_len, contig_seqs, means, regions):
    """the variants of the candidates whose first breakpoint lies on chrA (:238-541) from evidence handed in:
    means[(chrA, chrB, cluster)] = {"avg_a", "avg_b", "covM"} (tiddit_region.candidate_means; covM None where get_region gives it),
    regions[(chrom, start, end, bp)] = get_region's 6-tuple.  -> [[chrom, pos, vcf fields, scoring dict], ...] (QUAL unset)"""
    variants = []
    var_n = 0
    for chrB, cid, c, posA, posB, avg_a, avg_b in survivors(chrA, sv_clusters, args, library, means):
        n_discordants, n_splits, n_contigs = c["N_discordants"], c["N_splits"], c["N_contigs"]
        var_n += 1
        sample_data = {}
        for sample in samples:
            sample_data[sample] = site_evidence(chrA, chrB, posA, posB, c["startA"], c["endA"], c["startB"], c["endB"], regions,
                                                means[(chrA, chrB, cid)]["covM"])
        # `sample` is the last sample from here on, as in the reference
        inverted = non_inverted = 0
        pa, pb = c["positions_A"], c["positions_B"]
        for i in range(len(pa["orientation_discordants"])):
            if pa["orientation_discordants"][i] == pb["orientation_discordants"][i]:
                inverted += 1
            else:
                non_inverted += 1
        for kind in ("orientation_splits", "orientation_contigs"):
            for i in range(len(pa[kind])):
                if not pa[kind][i] == pb[kind][i]:
                    inverted += 1
                else:
                    non_inverted += 1
        svtype, cn = find_sv_type(chrA, chrB, inverted, non_inverted, args, sample_data, samples, library)
        last = sample_data[sample]
        filt = sv_filter(sample_data, args, chrA, chrB, posA, posB, max_ins_len, n_discordants, n_splits, library, last["discA"], last["discB"],
                         last["splitA"], last["splitB"], n_contigs)
        for sample in samples:                 # read-depth overrides of the filter
            sd = sample_data[sample]
            covA, covM, covB = sd["covA"], sd["covM"], sd["covB"]
            if "DEL" in svtype:
                if cn == 0:
                    filt = "PASS"
                if covA > covM * (cn + 0.9) and covB > covM * (cn + 0.9):
                    filt = "PASS"
            elif "DUP" in svtype and filt == "BelowExpectedLinks":
                filt = "PASS"
            scoring_dict = {"n_contigs": n_contigs, "n_discordants": n_discordants, "n_splits": n_splits, "covA": covA, "covM": covM, "covB": covB,
                            "refRA": sd["refRA"], "refRB": sd["refRB"], "refFA": sd["refFA"], "refFB": sd["refFB"]}
        last = sample_data[sample]
        regions_info = ["REGIONA={},{}".format(c["startA"], c["endA"]), "REGIONB={},{}".format(c["startB"], c["endB"]),
                        "LFA={},{}".format(last["discA"], last["splitA"])]
        if svtype != "BND":
            info = ["SVTYPE={}".format(svtype), "SVLEN={}".format(posB - posA), "END={}".format(posB)] + regions_info
            info += ["LFB={},{}".format(last["discB"], last["splitB"]), "LTE={},{}".format(n_discordants, n_splits), _ctg(c, n_contigs, contig_seqs)]
            alt = "<{}>".format(svtype)
            variant = [chrA, str(posA), "SV_{}_1".format(var_n), "N", alt, ".", filt, ";".join(info), FORMAT_COL]
            for sample in samples:
                sd = sample_data[sample]
                GT = depth_genotype(_genotype(c, sd, sample, args, n_contigs), svtype, cn, library["contig_ploidy_{}".format(chrA)])
                variant.append(_sample_column(GT, cn, sd, n_discordants, n_splits))
            variants.append([chrA, posA, variant, scoring_dict])
            continue
        # a break end: two records.  `inverted` is reset before it is compared (:432-439), so the alt strings never take the inverted forms
        info = ["SVTYPE=BND"] + regions_info
        info += ["LFB={},{}".format(last["discA"], last["splitA"]), "LTE={},{}".format(n_discordants, n_splits), _ctg(c, n_contigs, contig_seqs)]
        inverted = False
        before = posA != c["endA"]
        if inverted > non_inverted:
            inverted = True
        if not inverted and not before:
            alt_a, alt_b = "N[{}:{}[".format(chrB, posB), "]{}:{}]N".format(chrA, posA)
        elif not inverted and before:
            alt_a, alt_b = "]{}:{}]N".format(chrB, posB), "N[{}:{}[".format(chrA, posA)
        elif inverted and not before:
            alt_a, alt_b = "N]{}:{}]".format(chrB, posB), "[{}:{}[N".format(chrA, posA)
        else:
            alt_a, alt_b = "[{}:{}[N".format(chrB, posB), "N]{}:{}]".format(chrA, posA)
        info = ";".join(info)
        for chrom, pos, suffix, alt in ((chrA, posA, 1, alt_a), (chrB, posB, 2, alt_b)):
            variant = [chrom, str(pos), "SV_{}_{}".format(var_n, suffix), "N", alt, ".", filt, info, FORMAT_COL]
            for sample in samples:
                sd = sample_data[sample]
                variant.append(_sample_column(_genotype(c, sd, sample, args, n_contigs), cn, sd, n_discordants, n_splits))
            variants.append([chrom, pos, variant, scoring_dict])
    return variants


def finish(sv_clusters, variants_list):
    """percentiles of the support ratios over every variant, QUAL of each, the variants dict of main (:571-593)"""
    variants = {}
    for chrA in sv_clusters:
        variants[chrA] = []
        for chrB in sv_clusters[chrA]:
            variants[chrB] = []
    ratios = {"fragments_A": [], "fragments_B": [], "reads_A": [], "reads_B": []}
    for v in variants_list:
        for variant in v:
            d = variant[3]
            if d["n_discordants"]:
                ratios["fragments_A"].append(d["n_discordants"] / (d["refFA"] + d["n_discordants"]))
                ratios["fragments_B"].append(d["n_discordants"] / (d["refFB"] + d["n_discordants"]))
            if d["n_splits"]:
                ratios["reads_A"].append(d["n_splits"] / (d["refRA"] + d["n_splits"]))
                ratios["reads_B"].append(d["n_splits"] / (d["refRB"] + d["n_splits"]))
    percentiles = {"FA": percentile(ratios["fragments_A"], PERCENTILES), "FB": percentile(ratios["fragments_B"], PERCENTILES),
                   "RA": percentile(ratios["reads_A"], PERCENTILES), "RB": percentile(ratios["reads_B"], PERCENTILES)}
    for v in variants_list:
        for variant in v:
            variant[2][5] = str(scoring(variant[3], percentiles))
            variants[variant[0]].append([variant[1], variant[2]])
    return variants


def type_variants(sv_clusters, args, library, samples, max_ins_len, contig_seqs, means, regions):
    """the typing layer on its own: evidence in, the variants dict out"""
    return finish(sv_clusters, [define_variant(chrA, sv_clusters, args, library, samples, max_ins_len, contig_seqs, means, regions)
                                for chrA in sv_clusters])


def vcf_body(contigs, variants):
    """the records as the driver writes them (__main__.py:201-207): contig by contig, each sorted (stably) on position"""
    lines = []
    for chrom in contigs:
        if chrom not in variants:
            continue
        for variant in sorted(variants[chrom], key=lambda x: x[0]):
            lines.append("\t".join(variant[1]) + "\n")
    return "".join(lines)


# the store the signal scan of this process filled (tiddit_signal sets it; the variant stage frees it — or, with KEEP_STORE, hands it
# back here for the stage behind it: TIDDIT_GENOTYPE, whose driver frees it)
LIVE_STORE = None
KEEP_STORE = False
STAGE_SECONDS = {}


def take_store(bam_file_name, min_q, max_ins):
    """the live store when it holds this file under these parameters, else None (a store for anything else is freed)"""
    global LIVE_STORE
    import os
    s = LIVE_STORE
    LIVE_STORE = None
    if s is None:
        return None
    if os.path.abspath(s.path) == os.path.abspath(bam_file_name) and s.min_q == int(min_q) and s.max_ins == int(max_ins):
        return s
    s.close()
    return None


def evidence(store, queries, min_q, max_ins):
    """every (chrom, start, end, bp) of queries -> get_region's 6-tuple, from one launch over the store"""
    keys = list(dict.fromkeys(queries))
    if not keys:
        return {}
    rows = numpy.array([(store.tid[ch], s, e, bp) for ch, s, e, bp in keys], dtype=numpy.int64)
    counts = store.region_counts(rows, min_q, max_ins)
    return {k: region_tuple(counts[i], k[1], k[2]) for i, k in enumerate(keys)}


def _prepare(bam_file_name, sv_clusters, args, library, coverage_data, gc, T):
    """the host side before the counts: the assembly contigs, the coverage means of every candidate, the get_region calls of the
    candidates that pass the pre-filters -> (contig_seqs, means, queries)"""
    import time
    t = time.time()
    contig_seqs = {}
    if not args.skip_assembly:
        name = None
        for line in open("{}_tiddit/clips.fa.assembly.clean.mag".format(args.o)):
            if line[0] == ">":
                name = line[1:].rstrip()
            else:
                contig_seqs[name] = line.strip("\n")
    means = tiddit_region.candidate_means(sv_clusters, coverage_data, gc, library)
    T["candidate means (device)"] = time.time() - t
    t = time.time()
    queries = []
    for chrA in sv_clusters:
        for chrB, cid, c, posA, posB, _, _ in survivors(chrA, sv_clusters, args, library, means):
            queries += region_queries(chrA, chrB, c, posA, posB)
    T["pre-filters (host)"] = time.time() - t
    return contig_seqs, means, queries


def main(bam_file_name, sv_clusters, args, library, min_mapq, samples, coverage_data, contig_number, max_ins_len, gc):
    import time
    T = STAGE_SECONDS
    T.clear()
    contig_seqs, means, queries = _prepare(bam_file_name, sv_clusters, args, library, coverage_data, gc, T)
    t = time.time()
    store = take_store(bam_file_name, min_mapq, int(max_ins_len))
    if store is None:
        store = tiddit_region.build_store(bam_file_name, min_mapq, int(max_ins_len))
        T["evidence store (one ingest pass)"] = time.time() - t
        t = time.time()
    try:
        regions = evidence(store, queries, min_mapq, int(max_ins_len))
    except BaseException:
        store.close()
        raise
    if KEEP_STORE:
        global LIVE_STORE
        LIVE_STORE = store
    else:
        store.close()
    T["region counts (device, one launch)"] = time.time() - t
    t = time.time()
    out = type_variants(sv_clusters, args, library, samples, max_ins_len, contig_seqs, means, regions)
    T["typing + scoring (host)"] = time.time() - t
    return out


# ---- N ranks: every rank holds the store of its own shard of the file ---------------------------------------------------------
# Every record is in exactly one rank's store, and all seven sums of a query are order-independent integer sums over the records
# its region fetch returns (each shard's range and max span are its own), so the counts of one query over the N stores add up to the
# counts over the whole file's store: rank 0 broadcasts all the queries, every rank answers them in one launch, one int64 SUM-reduce.

def _broadcast_abort(group=None):
    """rank 0 failed before it had queries: nq = -1 tells the other ranks (who wait in evidence_sharded's first broadcast)"""
    import torch
    import torch.distributed as dist
    from . import dist as tdist
    dist.broadcast(torch.tensor([-1], dtype=torch.int64, device=tdist._wire_device(group)), 0, group=group)


def evidence_sharded(store, queries, min_q, max_ins, group=None):
    """:func:`evidence` on N ranks, a collective: every rank calls it with the store of its shard (anything with ``.tid`` on rank 0
    and ``region_counts`` — or ``region_counts_device`` over nccl); rank 0 passes its (chrom, start, end, bp) list, the other ranks
    None.  nq, then the int32[nq][4] rows are broadcast (device tensors over nccl, host tensors over gloo); every rank answers all of
    them over its store; the int64 counts, plus one word counting the ranks whose counts call failed, are SUM-reduced to rank 0.
    -> the regions dict on rank 0, None elsewhere.  No failure leaves a rank waiting: rank 0 broadcasts nq = -1 when it cannot
    make the rows, and every rank joins the reduce whether its own call failed or not."""
    import torch
    import torch.distributed as dist
    from . import dist as tdist
    rank = dist.get_rank(group)
    dev = tdist._wire_device(group)
    keys = rows = None
    if rank == 0:
        try:
            keys = list(dict.fromkeys(queries))
            rows = numpy.array([(store.tid[ch], s, e, bp) for ch, s, e, bp in keys], dtype=numpy.int32).reshape(-1, 4)
        except BaseException:
            _broadcast_abort(group)
            raise
    n = torch.tensor([len(keys) if rank == 0 else 0], dtype=torch.int64, device=dev)
    dist.broadcast(n, 0, group=group)
    nq = int(n.item())
    if nq < 0:
        store.close()
        raise RuntimeError("evidence_sharded: rank 0 failed before it broadcast the queries")
    if nq == 0:
        return {} if rank == 0 else None
    q = torch.from_numpy(rows).to(dev) if rank == 0 else torch.empty((nq, 4), dtype=torch.int32, device=dev)
    dist.broadcast(q, 0, group=group)
    out = torch.zeros(nq * 7 + 1, dtype=torch.int64, device=dev)
    failed = None
    try:
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)                  # (the broadcast ran on torch's streams, the library runs on its own)
            store.region_counts_device(q.data_ptr(), nq, min_q, max_ins, out.data_ptr())
        else:
            out[:nq * 7] = torch.from_numpy(numpy.ascontiguousarray(store.region_counts(q.numpy(), min_q, max_ins), dtype=numpy.int64).reshape(-1))
    except Exception as e:
        failed = e
        out.zero_()
        out[-1] = 1
    dist.reduce(out, 0, op=dist.ReduceOp.SUM, group=group)
    if failed is not None:
        raise failed
    if rank != 0:
        return None
    total = out.cpu().numpy()
    if total[-1]:
        raise RuntimeError("evidence_sharded: the region counts failed on %d other rank(s)" % int(total[-1]))
    counts = total[:-1].reshape(nq, 7)
    return {k: region_tuple(counts[i], k[1], k[2]) for i, k in enumerate(keys)}


def main_sharded(bam_file_name, sv_clusters, args, library, min_mapq, samples, coverage_data, contig_number, max_ins_len, gc, group=None):
    """:func:`main` on N ranks (torch.distributed initialised; nccl = RCCL, or gloo), called by every rank: rank 0 computes the means,
    the pre-filters and the typing from its arguments (the other ranks' may be anything); every rank answers the queries over the
    store of its shard — the one its scan left (LIVE_STORE), else one built by a pass over its shard of the file.
    -> the variants dict on rank 0, None elsewhere."""
    import time
    import torch.distributed as dist
    from . import dist as tdist
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    T = STAGE_SECONDS
    T.clear()
    t = time.time()
    store = take_store(bam_file_name, min_mapq, int(max_ins_len))
    try:
        if store is None:
            store = tiddit_region.build_store(bam_file_name, min_mapq, int(max_ins_len), shard=(rank, world))
            tdist.check_seams(*store.seam, group=group)
            T["evidence store (one ingest pass over this rank's shard)"] = time.time() - t
        contig_seqs = means = queries = None
        if rank == 0:
            try:
                contig_seqs, means, queries = _prepare(bam_file_name, sv_clusters, args, library, coverage_data, gc, T)
            except BaseException:
                _broadcast_abort(group)
                raise
        t = time.time()
        regions = evidence_sharded(store, queries, min_mapq, int(max_ins_len), group)
        T["region counts (N ranks: broadcast, one launch per rank, reduce)"] = time.time() - t
    finally:
        if store is not None:
            store.close()
    if rank != 0:
        return None
    t = time.time()
    out = type_variants(sv_clusters, args, library, samples, max_ins_len, contig_seqs, means, regions)
    T["typing + scoring (host)"] = time.time() - t
    return out
