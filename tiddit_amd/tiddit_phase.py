"""Read-backed phasing of the known SNV sites from the ``--sv`` scan (``TIDDIT_PHASE=1 | S | S:H``, only together with
``TIDDIT_ALLELES``): which heterozygous alleles of the sites file sit on the same chromosome copy, from the reads and read pairs that
cover two of them — ``{o}.phase.tab`` (a phased genotype and a phase set per heterozygous site) and ``{o}.phase.blocks.tab`` (one line
per phase block), from the one pass over the BAM.  The observation keys are stored on the device beside the allele counters
(csrc/tdt_phase.hip: ``phase_keys``, one launch per batch inside the allele handle's push) and reduced there once per job: fragment
rows, links, a maximum spanning forest, a check.  Every rule is an integer rule; this module is the specification and the device
result equals it bit for bit.

The switch.  ``S`` = the minimum link support, 1 ... 10^6, default 2; ``H`` = the minimum number of reads per allele for a site to be
heterozygous, 1 ... 10^6, default 3.  A bare ``1`` means the defaults; a support of 1 is written ``1:3``.  ``min_bq`` is
``TIDDIT_ALLELES_MIN_BQ``.  The switch without ``TIDDIT_ALLELES``, or any other value form, ends the job with an error before the scan;
so do N ranks (a fragment can straddle a shard seam).  Unset or empty is off: nothing is read, allocated or launched.

1  Phaseable sites.  A device site of :class:`tiddit_alleles.Sites` is phaseable when exactly one accepted row of the sites file lies at
   its position; it carries ``ref2`` / ``alt2``, the 2-bit codes (A C G T = 0 1 2 3) of that row's bases.  Its global index ``g`` is its
   index in the contig-major table, below 2^31.  Positions with several rows are never observed.
2  Reads that count: the gate, the well-formedness test and the CIGAR walk are :func:`tiddit_alleles.walk_read`'s.  In addition
   ``l_read_name >= 1`` (the name lies inside a well-formed record).  A malformed read gives nothing and adds one to ``malformed``;
   every other read that counts adds one to ``reads_used``.
3  Observations.  A phaseable site touched by ``M = X`` gives an observation when the quality byte is ``0xff`` or ``>= min_bq`` and the
   nibble is the site's REF (allele 0) or ALT (allele 1).  Every other base, ``D``, ``N`` and a low quality give none.  A read keeps its
   first 8 observations in walk order; a read that had more adds one to ``capped_reads``.
4  Keys.  ``K1 = fnv1a64(name bytes without the NUL) & (2^hash_bits - 1)`` (offset basis 0xcbf29ce484222325; per byte XOR, then times
   0x100000001b3 modulo 2^64); ``K2 = g << 1 | allele``.  ``hash_bits`` is 64 in every job.  Two names with equal ``K1`` ARE one fragment.
5  Fragment rows: the distinct ``(K1, g)`` with ``n`` observations, ``n_alt`` of them ALT.  A row is clean when ``n_alt`` is 0 or ``n``
   (overlapping mates that agree); otherwise it is dropped and counted in ``discordant_rows``.
6  Heterozygous sites, from the finished allele counters: phaseable, ``REF_N >= H``, ``ALT_N >= H`` and ``5 * min >= REF_N + ALT_N``.
7  Links.  Within one ``K1`` the clean rows at het sites ascending by ``g``: every consecutive pair on one contig is a link ``(i, j)``
   with parity ``allele_i ^ allele_j``; a pair on two contigs adds one to ``cross_contig_pairs`` and the walk goes on.  The link table
   is the distinct ``(j, i)`` ascending, each with ``N`` and ``TRANS`` (``CIS = N - TRANS``); ``row`` is a link's rank in that order.
8  A link is eligible when ``max(CIS, TRANS) >= S`` and ``4 * min <= max``; its parity is ``p = TRANS > CIS``, its weight
   ``w = min(max - min, 2^31 - 1)``.  The strict total order: larger ``w`` first, then smaller ``row``.  The others are ``weak_links``.
9  The forest is the maximum spanning forest of the eligible links under that order (Kruskal; unique).  A block is a component of two
   or more sites, its ``PS`` the 1-based POS of its lowest site; the phase of a site is the XOR of the parities on the forest path from
   the lowest site: ``GT`` ``0|1`` for phase 0, ``1|0`` for phase 1.  A het site in no block has ``0/1`` and PS ``.``.
10 Every eligible link outside the forest has both ends in one block: it AGREES when ``phase_i ^ phase_j == p``, else it is a
   CONFLICT; both are summed per block and over the job.

Files.  ``{o}.phase.tab``: ``# tiddit_amd phase v1 min_link=S min_allele=H min_bq=B hash=fnv1a64``, the ``SN name n`` rows (:data:`SN`),
then ``#CHROM POS REF ALT REF_N ALT_N GT PS`` per het site, ascending.  ``{o}.phase.blocks.tab``: ``#CHROM START END SITES EDGES AGREE
CONFLICT`` per block, ascending; EDGES = the block's eligible links (SITES - 1 forest edges + AGREE + CONFLICT).
"""
import bisect
import ctypes
import time

import numpy

from . import _native, tiddit_alleles

DEFAULT_MIN_LINK, DEFAULT_MIN_ALLELE, MAX_CUT = 2, 3, 10 ** 6
MAX_OBS = 8
FNV_BASIS, FNV_PRIME = 0xcbf29ce484222325, 0x100000001b3
PUSH = ("malformed", "reads_used", "observations", "capped_reads")
FINISH = ("fragment_rows", "discordant_rows", "cross_contig_pairs", "links", "weak_links", "forest_edges", "agree", "conflict", "phased_sites", "blocks")
SN = PUSH + ("phaseable_sites", "het_sites", "phased_sites", "blocks", "fragment_rows", "discordant_rows", "cross_contig_pairs", "links", "weak_links",
             "forest_edges", "agree", "conflict")
HEADER = "#CHROM\tPOS\tREF\tALT\tREF_N\tALT_N\tGT\tPS\n"
BLOCKS_HEADER = "#CHROM\tSTART\tEND\tSITES\tEDGES\tAGREE\tCONFLICT\n"
STAGE_SECONDS = {}
STAGE_NOTES = {}            # counts of the last main() that are not seconds


# ------------------------------------------------------------------------------------------- the switch and the sites
def parse_switch(value, alleles_on):
    """``TIDDIT_PHASE`` -> None (unset or empty) or ``(S, H)``; ValueError (its text is the error line) for a value that is none of the
    three forms and for the switch without ``TIDDIT_ALLELES``"""
    if value is None or value == "":
        return None

    def cut(text, what):
        if not text.isdigit() or str(int(text)) != text or not (1 <= int(text) <= MAX_CUT):
            raise ValueError("{} is an integer 1 ... 10^6".format(what))
        return int(text)
    parts = value.split(":")
    if len(parts) > 2:
        raise ValueError("the forms are 1, S and S:H")
    if len(parts) == 1:
        s = cut(parts[0], "the minimum link support")
        got = (DEFAULT_MIN_LINK if s == 1 else s, DEFAULT_MIN_ALLELE)
    else:
        got = (cut(parts[0], "the minimum link support"), cut(parts[1], "the minimum number of reads per allele"))
    if not alleles_on:
        raise ValueError("the sites are those of TIDDIT_ALLELES=sites.vcf: TIDDIT_ALLELES not set")
    return got


def site_codes(sites):
    """rule 1 -> uint8[device sites]: ``ref2 | alt2 << 2``, 0xff for a site that is not phaseable"""
    ns = len(sites)
    if ns >= 1 << 31:
        raise ValueError("{} sites; phasing keeps fewer than 2^31".format(ns))
    codes = numpy.full(ns, 0xff, dtype=numpy.uint8)
    if sites.rows:
        k = numpy.array([r[4] for r in sites.rows], dtype=numpy.int64)
        c = numpy.array(["ACGT".index(r[2]) | "ACGT".index(r[3]) << 2 for r in sites.rows], dtype=numpy.uint8)
        single = numpy.bincount(k, minlength=ns)[k] == 1
        codes[k[single]] = c[single]
    return codes


def het_flags(table, codes, min_allele):
    """rule 6 over the finished counters -> (uint8[sites] flags, REF_N, ALT_N); numpy, no loop"""
    table = numpy.asarray(table, dtype=numpy.int64).reshape(-1, 8)
    ok = codes != 0xff
    safe = numpy.where(ok, codes, 0).astype(numpy.int64)
    at = numpy.arange(len(codes))
    ref_n, alt_n = table[at, safe & 3], table[at, safe >> 2]
    lo = numpy.minimum(ref_n, alt_n)
    het = ok & (ref_n >= min_allele) & (alt_n >= min_allele) & (5 * lo >= ref_n + alt_n)
    return het.astype(numpy.uint8), ref_n, alt_n


# ------------------------------------------------------------------------------------------- the definition
def fnv1a64(name):
    h = FNV_BASIS
    for b in bytes(name):
        h = ((h ^ b) * FNV_PRIME) & 0xffffffffffffffff
    return h


def keys_of_read(keys, sn, codes, hash_bits, site_pos, site_off, tid, pos, end, mapq, flag, rec_off, raw, min_q, min_bq):
    """THE DEFINITION, one read (rules 2 - 4): appends its ``(K1, K2)`` to ``keys`` and adds to the push counters ``sn``"""
    got = tiddit_alleles.walk_read(site_pos, site_off, tid, pos, end, mapq, flag, rec_off, raw, min_q)
    if got is None:
        return
    if got is tiddit_alleles.MALFORMED or got[1] < 1:
        sn["malformed"] += 1
        return
    name_off, l_name, touches = got
    sn["reads_used"] += 1
    obs = []
    for k, op, nib, ql in touches:
        c = int(codes[k])
        if c == 0xff or op != 0 or not (ql == 0xff or ql >= min_bq):
            continue
        if nib == 1 << (c & 3):
            obs.append(k << 1)
        elif nib == 1 << (c >> 2):
            obs.append(k << 1 | 1)
    if len(obs) > MAX_OBS:
        sn["capped_reads"] += 1
        obs = obs[:MAX_OBS]
    if obs:
        k1 = fnv1a64(raw[name_off:name_off + l_name - 1]) & ((1 << hash_bits) - 1)
        keys.extend((k1, o) for o in obs)
        sn["observations"] += len(obs)


def keys_of_batch(keys, sn, codes, hash_bits, site_pos, site_off, b, min_q, min_bq):
    """rules 2 - 4 over one batch (an object with the columns ``tid pos end mapq flag rec_off`` and ``raw``)"""
    raw = b.raw if isinstance(b.raw, (bytes, bytearray)) else memoryview(numpy.ascontiguousarray(b.raw))
    site_pos = [int(x) for x in site_pos]
    for i in range(len(b.tid)):
        keys_of_read(keys, sn, codes, hash_bits, site_pos, site_off, int(b.tid[i]), int(b.pos[i]), int(b.end[i]), int(b.mapq[i]), int(b.flag[i]),
                     int(b.rec_off[i]), raw, min_q, min_bq)


def new_counters():
    return {k: 0 for k in PUSH}


def links_of_keys(keys, het, site_off):
    """rules 5 and 7 -> (j, i, N, TRANS) as four lists in (j, i) order, and the counters fragment_rows discordant_rows cross_contig_pairs"""
    rows = {}
    for k1, k2 in keys:
        e = rows.setdefault((k1, k2 >> 1), [0, 0])
        e[0] += 1
        e[1] += k2 & 1
    sn = {"fragment_rows": len(rows), "discordant_rows": 0, "cross_contig_pairs": 0}
    off = [int(x) for x in site_off]
    links, last = {}, None                                  # last = (K1, g, allele) of the walk's last clean het row
    for (k1, g), (n, n_alt) in sorted(rows.items()):
        if n_alt not in (0, n):
            sn["discordant_rows"] += 1
            continue
        if not het[g]:
            continue
        allele = int(n_alt != 0)
        if last is not None and last[0] == k1:
            if bisect.bisect_right(off, last[1]) == bisect.bisect_right(off, g):
                e = links.setdefault((g, last[1]), [0, 0])
                e[0] += 1
                e[1] += allele ^ last[2]
            else:
                sn["cross_contig_pairs"] += 1
        last = (k1, g, allele)
    order = sorted(links)
    return [k[0] for k in order], [k[1] for k in order], [links[k][0] for k in order], [links[k][1] for k in order], sn


def eligible(n, trans, min_link):
    """rule 8 -> (eligible, parity, weight)"""
    cis = n - trans
    hi, lo = max(cis, trans), min(cis, trans)
    return hi >= min_link and 4 * lo <= hi, int(trans > cis), min(hi - lo, (1 << 31) - 1)


def forest(n_sites, j, i, n, trans, min_link):
    """rules 8 - 10 on ANY link rows (row = the index) -> a dict: ``root`` int32[n_sites] (the block's lowest site, -1 in no block),
    ``phase`` uint8[n_sites], ``edge_used`` uint8[links], ``agree`` / ``conflict`` uint32[n_sites] at each block's lowest site, and the
    counters weak_links forest_edges agree conflict phased_sites blocks"""
    nl = len(j)
    parent, par = {}, {}                                    # union-find over the sites that have a link; par = parity against the parent

    def find(v):
        path = []
        while parent.setdefault(v, v) != v:
            path.append(v)
            v = parent[v]
        acc = 0
        for u in reversed(path):                            # (from the root down: parity against the root)
            acc ^= par.get(u, 0)
            parent[u], par[u] = v, acc
        return v
    cand = []
    weak = 0
    info = []
    for row in range(nl):
        ok, p, w = eligible(int(n[row]), int(trans[row]), min_link)
        info.append((ok, p))
        if ok:
            cand.append((-w, row))
        else:
            weak += 1
    used = numpy.zeros(nl, dtype=numpy.uint8)
    for _, row in sorted(cand):
        a, b = int(i[row]), int(j[row])
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra], par[ra] = rb, par.get(a, 0) ^ par.get(b, 0) ^ info[row][1]
            used[row] = 1
    root = numpy.full(n_sites, -1, dtype=numpy.int32)
    phase = numpy.zeros(n_sites, dtype=numpy.uint8)
    agree, conflict = numpy.zeros(n_sites, dtype=numpy.uint32), numpy.zeros(n_sites, dtype=numpy.uint32)
    def against_root(v):
        r = find(v)
        return r, (par[v] if v != r else 0)
    low = {}
    for v in sorted(parent):
        low.setdefault(find(v), v)                          # (ascending: the first site of a component is its lowest)
    for v in parent:
        r, pv = against_root(v)
        root[v], phase[v] = low[r], pv ^ against_root(low[r])[1]
    n_agree = n_conflict = 0
    for row in range(nl):
        if info[row][0] and not used[row]:
            a, b = int(i[row]), int(j[row])
            if int(phase[a]) ^ int(phase[b]) == info[row][1]:
                agree[root[a]] += 1
                n_agree += 1
            else:
                conflict[root[a]] += 1
                n_conflict += 1
    return {"root": root, "phase": phase, "edge_used": used, "agree": agree, "conflict": conflict,
            "sn": {"weak_links": weak, "forest_edges": int(used.sum()), "agree": n_agree, "conflict": n_conflict, "phased_sites": len(parent) if nl else 0,
                   "blocks": len(low)}}


def blocks_of(root, agree, conflict):
    """the per-site results -> (start, end, sites, edges, agree, conflict) per block, ascending (global site indices); numpy"""
    root = numpy.asarray(root)
    at = numpy.flatnonzero(root >= 0)
    start = numpy.unique(root[at]).astype(numpy.int32)
    which = numpy.searchsorted(start, root[at])
    sites = numpy.bincount(which, minlength=len(start)).astype(numpy.uint32)
    end = numpy.zeros(len(start), dtype=numpy.int32)
    numpy.maximum.at(end, which, at.astype(numpy.int32))
    ag, co = numpy.asarray(agree)[start].astype(numpy.uint32), numpy.asarray(conflict)[start].astype(numpy.uint32)
    return start, end, sites, (sites - 1 + ag + co).astype(numpy.uint32), ag, co


def summarise(keys, het, site_off, min_link):
    """THE DEFINITION, one job (rules 5 - 10): the keys of every read, the het flags of rule 6 -> a dict: ``links`` = (j, i, N, TRANS,
    edge_used) arrays, ``root``, ``phase``, ``blocks`` (:func:`blocks_of`) and ``sn`` = the finish counters"""
    j, i, n, trans, sn = links_of_keys(keys, het, site_off)
    f = forest(len(het), j, i, n, trans, min_link)
    sn = dict(sn, links=len(j), **f["sn"])
    u32 = lambda x: numpy.array(x, dtype=numpy.uint32)
    return {"links": (u32(j), u32(i), u32(n), u32(trans), f["edge_used"]), "root": f["root"], "phase": f["phase"],
            "blocks": blocks_of(f["root"], f["agree"], f["conflict"]), "sn": sn}


# ------------------------------------------------------------------------------------------- the device side
def device_keys(counter):
    """the observation store of an :class:`tiddit_alleles.AlleleCounter` made with ``phase=`` -> (K1, K2) uint64, in store order"""
    lib, n = counter.ctx.lib, ctypes.c_size_t(0)
    _native.check(lib.tdt_alleles_phase_keys(counter.handle, None, None, ctypes.byref(n)))
    k1, k2 = numpy.zeros(n.value, dtype=numpy.uint64), numpy.zeros(n.value, dtype=numpy.uint64)
    _native.check(lib.tdt_alleles_phase_keys(counter.handle, _native.ptr(k1), _native.ptr(k2), ctypes.byref(n)))
    return k1, k2


def device_finish(counter, het, min_link):
    """``tdt_alleles_phase_finish`` and its read-outs -> the dict of :func:`summarise`, with the push counters in ``sn`` too and
    ``rounds`` = the Boruvka rounds run"""
    lib, h, P = counter.ctx.lib, counter.handle, _native.ptr
    het = numpy.ascontiguousarray(het, dtype=numpy.uint8)
    ns = counter.n_sites
    got = numpy.zeros(len(PUSH) + len(FINISH) + 1, dtype=numpy.uint64)
    _native.check(lib.tdt_alleles_phase_finish(h, P(het), int(min_link), P(got)))
    root, phase = numpy.zeros(ns, dtype=numpy.int32), numpy.zeros(ns, dtype=numpy.uint8)
    _native.check(lib.tdt_alleles_phase_sites(h, P(root), P(phase), ns))
    n = ctypes.c_size_t(0)
    _native.check(lib.tdt_alleles_phase_links(h, None, None, None, None, None, ctypes.byref(n)))
    links = [numpy.zeros(n.value, dtype=numpy.uint32) for _ in range(4)] + [numpy.zeros(n.value, dtype=numpy.uint8)]
    _native.check(lib.tdt_alleles_phase_links(h, *[P(x) for x in links], ctypes.byref(n)))
    _native.check(lib.tdt_alleles_phase_blocks(h, None, None, None, None, None, None, ctypes.byref(n)))
    blocks = [numpy.zeros(n.value, dtype=numpy.int32) for _ in range(2)] + [numpy.zeros(n.value, dtype=numpy.uint32) for _ in range(4)]
    _native.check(lib.tdt_alleles_phase_blocks(h, *[P(x) for x in blocks], ctypes.byref(n)))
    names = PUSH + FINISH
    return {"links": tuple(links), "root": root, "phase": phase, "blocks": tuple(blocks), "sn": {k: int(got[x]) for x, k in enumerate(names)},
            "rounds": int(got[len(names)])}


def device_timing(counter):
    """-> (ms5 of the last finish, (asks, grows, capacity) of the observation store)"""
    ms, st = numpy.zeros(5), numpy.zeros(3, dtype=numpy.uint64)
    _native.check(counter.ctx.lib.tdt_alleles_phase_timing(counter.handle, _native.ptr(ms)))
    _native.check(counter.ctx.lib.tdt_alleles_phase_reserve_stats(counter.handle, _native.ptr(st)))
    return ms, tuple(int(x) for x in st)


def device_forest(n_sites, j, i, n, trans, min_link, ctx=None):
    """``tdt_phase_forest`` on host columns -> root, phase, edge_used, agree, conflict"""
    ctx = ctx or _native.default_context()
    P = _native.ptr
    j, i = numpy.ascontiguousarray(j, dtype=numpy.int32), numpy.ascontiguousarray(i, dtype=numpy.int32)
    n, trans = numpy.ascontiguousarray(n, dtype=numpy.uint32), numpy.ascontiguousarray(trans, dtype=numpy.uint32)
    root, phase = numpy.zeros(n_sites, dtype=numpy.int32), numpy.zeros(n_sites, dtype=numpy.uint8)
    used = numpy.zeros(len(j), dtype=numpy.uint8)
    agree, conflict = numpy.zeros(n_sites, dtype=numpy.uint32), numpy.zeros(n_sites, dtype=numpy.uint32)
    _native.check(ctx.lib.tdt_phase_forest(ctx.handle, P(j), P(i), P(n), P(trans), len(j), n_sites, int(min_link), P(root), P(phase), P(used), P(agree),
                                           P(conflict)))
    return root, phase, used, agree, conflict


# ------------------------------------------------------------------------------------------- the files
def file_text(sites, codes, het, ref_n, alt_n, result, push, names, min_link, min_allele, min_bq):
    """-> (the text of ``{o}.phase.tab``, of ``{o}.phase.blocks.tab``, the SN counters as a dict)"""
    site_pos, site_off = numpy.asarray(sites.site_pos), numpy.asarray(sites.site_off)
    root, phase = result["root"], result["phase"]
    sn = dict(push)
    sn.update(result["sn"])
    sn["phaseable_sites"], sn["het_sites"] = int((codes != 0xff).sum()), int(numpy.count_nonzero(het))
    head = "# tiddit_amd phase v1 min_link={} min_allele={} min_bq={} hash=fnv1a64\n".format(min_link, min_allele, min_bq)
    head += "".join("SN\t{}\t{}\n".format(k, sn[k]) for k in SN)
    at = numpy.flatnonzero(het)
    chrom = numpy.searchsorted(site_off, at, side="right") - 1
    letters = numpy.array(list("ACGT"))
    gt = numpy.where(root[at] < 0, "0/1", numpy.where(phase[at] == 0, "0|1", "1|0"))
    ps = numpy.where(root[at] < 0, ".", (site_pos[numpy.maximum(root[at], 0)].astype(numpy.int64) + 1).astype(str))
    cols = ([names[c] for c in chrom.tolist()], (site_pos[at].astype(numpy.int64) + 1).tolist(), letters[codes[at] & 3].tolist(),
            letters[codes[at] >> 2].tolist(), ref_n[at].tolist(), alt_n[at].tolist(), gt.tolist(), ps.tolist())
    body = "".join(map("%s\t%d\t%s\t%s\t%d\t%d\t%s\t%s\n".__mod__, zip(*cols)))
    start, end, n_sites, edges, agree, conflict = result["blocks"]
    bchrom = numpy.searchsorted(site_off, start, side="right") - 1
    bcols = ([names[c] for c in bchrom.tolist()], (site_pos[start].astype(numpy.int64) + 1).tolist(), (site_pos[end].astype(numpy.int64) + 1).tolist(),
             n_sites.tolist(), edges.tolist(), agree.tolist(), conflict.tolist())
    blocks = BLOCKS_HEADER + "".join(map("%s\t%d\t%d\t%d\t%d\t%d\t%d\n".__mod__, zip(*bcols)))
    return head + HEADER + body, blocks, sn


def summary_line(sn):
    return ("phase: {het_sites} het sites of {phaseable_sites} phaseable, {phased_sites} phased in {blocks} blocks; {links} links ({weak_links} weak), "
            "{forest_edges} forest edges, agree {agree}, conflict {conflict}; {observations} observations, discordant rows {discordant_rows}").format(**sn)


def write_files(prefix, text, blocks):
    with open(prefix + ".phase.tab", "w") as f:
        f.write(text)
    with open(prefix + ".phase.blocks.tab", "w") as f:
        f.write(blocks)


def main(counter, sites, table, prefix, names=None):
    """the stage behind :func:`tiddit_alleles.main` (which left the counter open): het flags from the counter table (numpy), the finish on
    the device, the two files and the summary line.  ``counter.phase`` = (site codes, capacity, hash_bits, S, H)."""
    STAGE_SECONDS.clear()
    STAGE_NOTES.clear()
    codes, _, _, min_link, min_allele = counter.phase
    t = time.time()
    het, ref_n, alt_n = het_flags(table, codes, min_allele)
    STAGE_SECONDS["phase het flags (host)"] = time.time() - t
    t = time.time()
    try:
        result = device_finish(counter, het, min_link)
        ms, (asks, grows, cap) = device_timing(counter)
    finally:
        counter.close()                                     # (also when the finish fails: the handle's HBM goes back)
    STAGE_NOTES.update({"phase store: reserves that asked the device": asks, "phase store: growths": grows, "phase store: capacity (keys)": cap,
                        "phase forest: rounds": result["rounds"]})
    STAGE_SECONDS["phase finish (device)"] = time.time() - t
    for k, name in enumerate(("fragment rows", "link keys", "link rows", "forest, check, sites")):
        STAGE_SECONDS["  phase " + name] = ms[k] * 1e-3
    t = time.time()
    push = {k: result["sn"][k] for k in PUSH}
    if names is None:
        seen = {}
        for r in sites.rows:                                # (a contig with a site has a row that names it)
            seen.setdefault(int(numpy.searchsorted(sites.site_off, r[4], side="right")) - 1, r[0])
        names = [seen.get(c, ".") for c in range(len(sites.site_off) - 1)]
    text, blocks, sn = file_text(sites, codes, het, ref_n, alt_n, result, push, names, min_link, min_allele, counter.min_bq)
    write_files(prefix, text, blocks)
    STAGE_SECONDS["phase tables text (host)"] = time.time() - t
    print(summary_line(sn))
    return result
