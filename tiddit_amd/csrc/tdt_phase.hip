// Read-backed phasing of the known SNV sites for gfx950 (TIDDIT_PHASE): which heterozygous alleles of the TIDDIT_ALLELES sites lie on the
// same chromosome copy, from the reads and read pairs that cover two of them.  The definition is tiddit_phase.py's; every result here is an
// order-independent integer (a count of equal keys, a maximum under a strict total order), so it equals the definition exactly.
//   * phase_keys — ONE launch per batch inside the allele handle's push, beside al_count, on the same columns and record bytes.  Lane =
//     read for the gate (ks_read_gate) and al_count's two lower bounds into the contig's sites; the reads with a site in reach are
//     compacted once more.  Lane = compacted read: the record is bounded in al_count's order of tests (rule 2 of the definition makes
//     that order binding: a record without a CIGAR is not malformed whatever its block_size says, and a negative pos is no reason to
//     refuse; KS_OPEN decides both otherwise, so the bound is spelled out with TDT_REC_* here), its CIGAR walked ONCE for all of its
//     sites, the first PH_MAX_OBS observations kept in registers, its name hashed (FNV-1a, 64 bit), and the keys K1 = hash, K2 = g << 1 |
//     allele staged in LDS (PH_BLOCK x 8 keys x 16 B = 32 KB) and appended with ks_stage / ks_flush: ONE atomic per workgroup.
//   * the finish, once per job: ks_finish on the observation store (rows = the distinct (K1, g) with n and n_alt); phase_links, lane = row,
//     looks ahead inside its K1 run for the next clean heterozygous row and stages L1 = j << 32 | i, L2 = parity into a SECOND store;
//     ks_finish on that one gives the link rows (N, TRANS) in (j, i) order; then the graph stage below.
//   * the graph stage (pf_*; also the generic entries tdt_phase_forest / tdt_phase_forest_device, on any link rows): Boruvka rounds in
//     plain launches — pf_pick: every component takes the maximum of w << 32 | (2^32 - 1 - row) over its outgoing eligible links by
//     atomicMax; pf_hook: a root hooks to the component at the other end of its pick (a mutual pick: only the larger label hooks), the
//     parity of the hooked root against its new root carried in bit 0 of the label word; pf_apply; pf_jump: label and parity, ONE 32-bit
//     word per site, flattened by pointer jumping until a launch changes nothing.  Rounds repeat until one hooks nothing.  No workgroup
//     waits for another.  pf_low / pf_check / pf_sites: the lowest site of every component, agree / conflict of the eligible links
//     outside the forest in the block's slot, and per site (root g or -1, phase against the lowest site).
// The compiler's resource report (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage) stands in the README row.
#include "tdt_keystore.h"
#include "tdt_phase.h"
#include <chrono>

typedef unsigned long long ull;

#define PH_BLOCK 256
#define PH_MAX_OBS TDT_PHASE_MAX_OBS
#define PHL_TILE 256                          // the rows of a phase_links workgroup: lane = row
#define PF_BLOCK 256
#define PF_NONE 0xffffffffu
#define PF_MAX_ROUNDS 64                      // (a round at least halves the components that still have an outgoing link: 31 suffice)
static_assert(PH_BLOCK == KS_BLOCK && PHL_TILE == KS_BLOCK && PH_MAX_OBS == 8, "a read's observations are eight registers; the staged keys are 256 x 8 x 16 B");

enum { PK_MALFORMED = 0, PK_USED, PK_OBS, PK_CAPPED, PK_N, PK_OR1 = PK_N };       // the push counters of the observation store
enum { LK_DISCORDANT = 0, LK_CROSS, LK_N, LK_OR1 = LK_N };                                      // ... of the link store
enum { PF_HOOKS = 0, PF_WEAK, PF_AGREE, PF_CONFLICT, PF_PHASED, PF_BLOCKS, PF_EDGES, PF_CHANGED, PF_CNT_N = 16 };
static_assert(PK_OR1 + 4 <= KS_N && LK_OR1 + 4 <= KS_N && PK_N == TDT_PHASE_PUSH_N && PK_N + 11 == TDT_PHASE_GOT_N, "state layout");

struct ph_table {                             // the kernel's view of the sites (device pointers)
    const int32_t *pos;
    const long long *off;
    const uint8_t *codes;                     // ref2 | alt2 << 2, 0xff: not phaseable
    int n_contigs;
};

struct pf_out {                               // what the graph stage writes (device pointers)
    int32_t *root;                            // ns: the block's lowest site, -1 in no block
    uint8_t *phase, *used;                    // ns; nl: the link is a forest edge
    uint32_t *agree, *conflict;               // ns: at the block's lowest site
};

struct tdt_phase {
    tdt_ctx *ctx;
    ph_table T;
    size_t ns;
    int min_q, min_bq;
    ull hash_mask;
    uint8_t *d_codes, *d_het;
    tdt_keystore S, L;                        // the observations (K1 = hash, K2 = g << 1 | allele); the links (L1 = j << 32 | i, L2 = parity)
    void *d_res;                              // the last finish's per-site results and edge flags
    size_t res_cap, n_links;
    pf_out R;
    bool done;                                // a finish since the last push or reset
    double ms[5];
};

__device__ __forceinline__ long long ph_lower_bound(const int32_t *__restrict__ s, long long lo, long long hi, int v) {
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (s[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(PH_BLOCK) void phase_keys(ks_cols I, const int32_t *__restrict__ endc, int n, ull raw_len, unsigned min_q, int min_bq, ph_table T,
                                                       ull hash_mask, ull *__restrict__ k1s, ull *__restrict__ k2s, ull cap, ull *__restrict__ st) {
    __shared__ ull s_k1[PH_BLOCK * PH_MAX_OBS], s_k2[PH_BLOCK * PH_MAX_OBS];                 // the workgroup's keys, in thread order
    __shared__ int s_read[PH_BLOCK], s_lo[PH_BLOCK], s_nin[PH_BLOCK];                         // the reads with a site in reach
    __shared__ int s_wsum[PH_BLOCK / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long first = (long long)blockIdx.x * PH_BLOCK, hi_read = first + PH_BLOCK < n ? first + PH_BLOCK : n;
    ull cnt[PK_N] = {0, 0, 0, 0};
    ull records = 0, eligible = 0;                                   // (the gate's own two counters are al_count's business, not a row here)
    ks_masks M;
    // ---- lane = read: the filters on the columns, the sites in [pos, end) as al_count finds them
    const ks_gated G = ks_read_gate<PH_BLOCK>(I, first, hi_read, min_q, records, eligible);
    int lo = 0, hi = 0;
    if (t < G.live) {
        const int c = I.tid[G.read];
        if (c < T.n_contigs) {
            const int p = I.pos[G.read], e = endc[G.read];
            const long long o0 = T.off[c], o1 = T.off[c + 1];
            if (o1 > o0 && e > p) {
                const long long a = ph_lower_bound(T.pos, o0, o1, p);
                if (a < o1 && T.pos[a] < e) {
                    lo = (int)a;
                    hi = (int)ph_lower_bound(T.pos, a + 1, o1, e);
                }
            }
        }
    }
    const bool has = hi > lo;
    const ull m_has = __ballot(has);
    const tdt_slots C = tdt_block_slots<PH_BLOCK / 64>(m_has, s_wsum, lane, wave);
    if (has) {
        const int k = C.base + tdt_lane_rank(m_has, lane);
        s_read[k] = G.read;
        s_lo[k] = lo;
        s_nin[k] = hi - lo;
    }
    __syncthreads();
    // ---- lane = compacted read: bound the record, walk its CIGAR once over its sites, keep the first eight observations
    const bool live = t < C.total;
    bool bad = false, used = false, over = false;
    unsigned ob[PH_MAX_OBS] = {0, 0, 0, 0, 0, 0, 0, 0};
    int nobs = 0;
    ull k1 = 0;
    const uint8_t *__restrict__ raw = I.raw;
    if (live) {
        const int ri = s_read[t];
        const int l0 = s_lo[t], l1 = l0 + s_nin[t];
        const int pos = I.pos[ri];
        const ull ro = I.rec_off[ri];
        bad = true;
        if (TDT_REC_HEADER_INSIDE(raw_len, ro)) {
            const tdt_rec R = TDT_REC_READ(raw, ro);
            if (R.n_cig == 0 || R.l_seq < 1) {                      // not a read that counts (and not a malformed one)
                bad = false;
            } else if (TDT_REC_FITS(R, raw_len)) {                  // (behind this everything read lies in [ro, ro + 4 + block_size))
                const uint8_t *cig = raw + R.cig(), *qual = raw + R.qual();
                const ull seq = R.seq();
                const unsigned n_cig = R.n_cig;
                const long long l_seq = R.l_seq;
                bad = R.l_name < 1;
                for (unsigned j = 0; j < n_cig; j++) bad |= (tdt_ld_u32(cig + 4ull * j) & 0xfu) > 8u;
                if (!bad) {
                    unsigned j = 0;
                    long long r = pos, q = 0;
                    for (int k = l0; k < l1 && !bad; k++) {
                        const long long s = T.pos[k];                // (ascending, >= pos: the walk only moves forward)
                        while (j < n_cig) {
                            const unsigned cw = tdt_ld_u32(cig + 4ull * j), op = cw & 0xfu;
                            const long long len = cw >> 4;
                            const bool ref = tdt_cig_on_ref(op);
                            if (ref && s < r + len) {
                                if (op != 2 && op != 3) {
                                    const long long qi = q + (s - r);
                                    if (qi >= l_seq) {
                                        bad = true;
                                    } else {
                                        const unsigned code = T.codes[k], ql = qual[qi];
                                        if (code != 0xffu && (ql == 0xffu || (int)ql >= min_bq)) {
                                            const unsigned nib = tdt_rec_base(raw, seq, (ull)qi);
                                            const int a = nib == (1u << (code & 3u)) ? 0 : nib == (1u << ((code >> 2) & 3u)) ? 1 : -1;
                                            if (a >= 0) {
                                                const unsigned key = ((unsigned)k << 1) | (unsigned)a;
#pragma unroll
                                                for (int x = 0; x < PH_MAX_OBS; x++)
                                                    if (x == nobs) ob[x] = key;
                                                over |= nobs >= PH_MAX_OBS;
                                                nobs += nobs < PH_MAX_OBS ? 1 : 0;
                                            }
                                        }
                                    }
                                }
                                break;
                            }
                            if (ref) r += len;
                            if (tdt_cig_on_query(op)) q += len;
                            j++;
                        }
                    }
                    used = !bad;
                }
                if (bad) nobs = 0, over = false;
                if (nobs) {                                         // FNV-1a over the name without its NUL
                    ull h = 0xcbf29ce484222325ull;
                    const uint8_t *name = raw + ro + 36;
                    for (unsigned x = 0; x + 1 < R.l_name; x++) h = (h ^ (ull)name[x]) * 0x100000001b3ull;
                    k1 = h & hash_mask;
                }
            }
        }
    }
    cnt[PK_MALFORMED] += (ull)__popcll(__ballot(live && bad));
    cnt[PK_USED] += (ull)__popcll(__ballot(used));
    cnt[PK_CAPPED] += (ull)__popcll(__ballot(over));
    cnt[PK_OBS] = tdt_wave_reduce<tdt_sum>((ull)nobs);
    // ---- the keys into LDS at the slots the stage hands out, then the emit (tdt_keystore.h)
    int total;
    const int slot = ks_stage<PH_BLOCK>(nobs, &total);              // (+ nobs <= total <= 8 x PH_BLOCK)
#pragma unroll
    for (int x = 0; x < PH_MAX_OBS; x++) {
        if (x < nobs) {
            M.add(k1, (ull)ob[x]);
            s_k1[slot + x] = k1;
            s_k2[slot + x] = (ull)ob[x];
        }
    }
    ks_flush<PH_BLOCK, PK_N>(cnt, M, total, s_k1, s_k2, k1s, k2s, cap, st);
}

// the contig of global site g: the last c with off[c] <= g (off[0] = 0 <= g < off[n_contigs])
__device__ __forceinline__ int ph_contig_of(const long long *__restrict__ off, int n_contigs, long long g) {
    int lo = 0, hi = n_contigs;                                     // the first c in [0, n_contigs] with off[c] > g
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= g) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

// The links of the fragment rows (the observation store's finish: K1, g << 1, n, n_alt in key order), lane = row: a clean row at a het site
// looks ahead inside its K1 run for the next such row; the pair is a link when both lie on one contig.  Every g is a key phase_keys
// built: below ns.
__global__ __launch_bounds__(PHL_TILE) void phase_links(const ull *__restrict__ rk1, const ull *__restrict__ rk2, const unsigned *__restrict__ sup,
                                                        const unsigned *__restrict__ rev, int nrows, const uint8_t *__restrict__ het,
                                                        const long long *__restrict__ off, int n_contigs, ull *__restrict__ k1s, ull *__restrict__ k2s, ull cap,
                                                        ull *__restrict__ st) {
    __shared__ ull s_k1[PHL_TILE], s_k2[PHL_TILE];
    const int t = threadIdx.x;
    const long long x = (long long)blockIdx.x * PHL_TILE + t;
    bool emit = false, cross = false, disc = false;
    ull L1 = 0, L2 = 0;
    if (x < nrows) {
        const ull K = rk1[x];
        const unsigned g = (unsigned)(rk2[x] >> 1), n_ = sup[x], na = rev[x];
        disc = !(na == 0 || na == n_);
        if (!disc && het[g]) {
            for (long long y = x + 1; y < nrows && rk1[y] == K; y++) {
                const unsigned gb = (unsigned)(rk2[y] >> 1), nb = sup[y], nab = rev[y];
                if ((nab == 0 || nab == nb) && het[gb]) {
                    if (ph_contig_of(off, n_contigs, g) == ph_contig_of(off, n_contigs, gb)) {
                        emit = true;
                        L1 = ((ull)gb << 32) | (ull)g;
                        L2 = (ull)((na != 0) != (nab != 0));
                    } else {
                        cross = true;
                    }
                    break;
                }
            }
        }
    }
    ull cnt[LK_N];
    cnt[LK_DISCORDANT] = (ull)__popcll(__ballot(disc));
    cnt[LK_CROSS] = (ull)__popcll(__ballot(cross));
    ks_masks M;
    int total;
    const int slot = ks_stage<PHL_TILE>(emit ? 1 : 0, &total);
    if (emit) {
        M.add(L1, L2);
        s_k1[slot] = L1;
        s_k2[slot] = L2;
    }
    ks_flush<PHL_TILE, LK_N>(cnt, M, total, s_k1, s_k2, k1s, k2s, cap, st);
}

// ---- the graph stage: link rows ji = j << 32 | i with N and TRANS over ns sites
// rule 8: eligible, with the weight and the parity
__device__ __forceinline__ bool pf_eligible(unsigned N, unsigned T, unsigned S, unsigned *w, unsigned *p) {
    const unsigned C = N - T, mx = C > T ? C : T, mn = C > T ? T : C, d = mx - mn;
    *p = T > C ? 1u : 0u;
    *w = d > 0x7fffffffu ? 0x7fffffffu : d;
    return mx >= S && 4ull * mn <= (ull)mx;
}

// the generic entries' columns as rows; a row with an end outside [0, ns), two equal ends or TRANS > N raises *bad
__global__ __launch_bounds__(PF_BLOCK) void pf_pack(const int32_t *__restrict__ j, const int32_t *__restrict__ i, const uint32_t *__restrict__ N,
                                                    const uint32_t *__restrict__ T, int nl, int ns, ull *__restrict__ ji, ull *__restrict__ bad) {
    const int x = blockIdx.x * PF_BLOCK + threadIdx.x;
    if (x >= nl) return;
    const int a = i[x], b = j[x];
    if (a < 0 || b < 0 || a >= ns || b >= ns || a == b || T[x] > N[x]) {
        *bad = 1;
        ji[x] = 0;
        return;
    }
    ji[x] = ((ull)(unsigned)b << 32) | (ull)(unsigned)a;
}

__global__ __launch_bounds__(PF_BLOCK) void pf_init(int ns, unsigned *__restrict__ lp, unsigned *__restrict__ hook, int *__restrict__ low, int *__restrict__ size) {
    const int v = blockIdx.x * PF_BLOCK + threadIdx.x;
    if (v >= ns) return;
    lp[v] = (unsigned)v << 1;
    hook[v] = PF_NONE;
    low[v] = 0x7fffffff;
    size[v] = 0;
}

// lane = link row: an eligible link between two components offers its order key to both (the labels are flat: lp >> 1 is the root)
__global__ __launch_bounds__(PF_BLOCK) void pf_pick(const ull *__restrict__ ji, const unsigned *__restrict__ N, const unsigned *__restrict__ T, int nl, unsigned S,
                                                    const unsigned *__restrict__ lp, ull *__restrict__ best) {
    const int x = blockIdx.x * PF_BLOCK + threadIdx.x;
    if (x >= nl) return;
    unsigned w, p;
    if (!pf_eligible(N[x], T[x], S, &w, &p)) return;
    const ull e = ji[x];
    const unsigned li = lp[(unsigned)e] >> 1, lj = lp[(unsigned)(e >> 32)] >> 1;
    if (li == lj) return;
    const ull key = ((ull)w << 32) | (ull)(0xffffffffu - (unsigned)x);      // (w >= 1: an eligible link has max > min; 0 = no pick)
    atomicMax(&best[li], key);
    atomicMax(&best[lj], key);
}

// lane = site: a root with a pick hooks to the component at the other end — unless that one picked the same link and has the larger label
__global__ __launch_bounds__(PF_BLOCK) void pf_hook(const ull *__restrict__ ji, const unsigned *__restrict__ N, const unsigned *__restrict__ T, int ns, unsigned S,
                                                    const unsigned *__restrict__ lp, const ull *__restrict__ best, unsigned *__restrict__ hook,
                                                    uint8_t *__restrict__ used, ull *__restrict__ cnt) {
    const int v = blockIdx.x * PF_BLOCK + threadIdx.x;
    bool hooks = false;
    if (v < ns && lp[v] == ((unsigned)v << 1) && best[v]) {
        const ull key = best[v];
        const unsigned row = 0xffffffffu - (unsigned)key;
        const ull e = ji[row];
        const unsigned wi = lp[(unsigned)e], wj = lp[(unsigned)(e >> 32)];
        const unsigned other = (wi >> 1) == (unsigned)v ? wj >> 1 : wi >> 1;
        if (best[other] != key || (unsigned)v > other) {
            unsigned w, p;
            (void)pf_eligible(N[row], T[row], S, &w, &p);
            hook[v] = (other << 1) | ((wi ^ wj ^ p) & 1u);         // phase(v's root) = phase(other's root) ^ par_i ^ par_j ^ p
            used[row] = 1;
            hooks = true;
        }
    }
    const ull m = __ballot(hooks);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&cnt[PF_HOOKS], (ull)__popcll(m));
}

__global__ __launch_bounds__(PF_BLOCK) void pf_apply(int ns, unsigned *__restrict__ lp, unsigned *__restrict__ hook, ull *__restrict__ best) {
    const int v = blockIdx.x * PF_BLOCK + threadIdx.x;
    if (v >= ns) return;
    const unsigned h = hook[v];
    if (h != PF_NONE) lp[v] = h, hook[v] = PF_NONE;
    best[v] = 0;
}

// one step of pointer jumping.  A site's label and its parity against that label are ONE word, so whatever a lane reads of another site
// is a valid (ancestor, parity against it) pair, before or behind that site's own step.
__global__ __launch_bounds__(PF_BLOCK) void pf_jump(int ns, unsigned *lp, ull *__restrict__ cnt) {
    const int v = blockIdx.x * PF_BLOCK + threadIdx.x;
    if (v >= ns) return;
    const unsigned w = lp[v], l = w >> 1;
    if (l == (unsigned)v) return;
    const unsigned wl = lp[l];
    if ((wl >> 1) == l) return;
    lp[v] = (wl & ~1u) | ((w ^ wl) & 1u);
    cnt[PF_CHANGED] = 1;
}

__global__ __launch_bounds__(PF_BLOCK) void pf_low(int ns, const unsigned *__restrict__ lp, int *__restrict__ low, int *__restrict__ size) {
    const int v = blockIdx.x * PF_BLOCK + threadIdx.x;
    if (v >= ns) return;
    const unsigned l = lp[v] >> 1;
    atomicMin(&low[l], v);
    atomicAdd(&size[l], 1);
}

// lane = link row: an eligible link outside the forest agrees with the phases of its ends or conflicts, counted at the block's lowest site
__global__ __launch_bounds__(PF_BLOCK) void pf_check(const ull *__restrict__ ji, const unsigned *__restrict__ N, const unsigned *__restrict__ T, int nl, unsigned S,
                                                     const unsigned *__restrict__ lp, const uint8_t *__restrict__ used, const int *__restrict__ low,
                                                     uint32_t *__restrict__ agree, uint32_t *__restrict__ conflict, ull *__restrict__ cnt) {
    const int x = blockIdx.x * PF_BLOCK + threadIdx.x;
    bool weak = false, ok = false, no = false;
    if (x < nl) {
        unsigned w, p;
        if (!pf_eligible(N[x], T[x], S, &w, &p)) {
            weak = true;
        } else if (!used[x]) {
            const ull e = ji[x];
            const unsigned wi = lp[(unsigned)e], wj = lp[(unsigned)(e >> 32)];
            const int slot = low[wi >> 1];                          // (both ends in one component: the link lost against a path between them)
            ok = ((wi ^ wj) & 1u) == p;
            no = !ok;
            atomicAdd(ok ? &agree[slot] : &conflict[slot], 1u);
        }
    }
    const ull mw = __ballot(weak), mo = __ballot(ok), mn = __ballot(no);
    if ((threadIdx.x & 63) == 0) {
        if (mw) atomicAdd(&cnt[PF_WEAK], (ull)__popcll(mw));
        if (mo) atomicAdd(&cnt[PF_AGREE], (ull)__popcll(mo));
        if (mn) atomicAdd(&cnt[PF_CONFLICT], (ull)__popcll(mn));
    }
}

// lane = site: (root, phase) re-based on the block's lowest site; a component of one site is no block
__global__ __launch_bounds__(PF_BLOCK) void pf_sites(int ns, const unsigned *__restrict__ lp, const int *__restrict__ low, const int *__restrict__ size,
                                                     int32_t *__restrict__ root, uint8_t *__restrict__ phase, ull *__restrict__ cnt) {
    const int v = blockIdx.x * PF_BLOCK + threadIdx.x;
    bool in = false, head = false;
    if (v < ns) {
        const unsigned w = lp[v], l = w >> 1;
        in = size[l] >= 2;
        const int b = in ? low[l] : -1;
        head = b == v;
        root[v] = b;
        phase[v] = in ? (uint8_t)((w ^ lp[b]) & 1u) : (uint8_t)0;
    }
    const ull mi = __ballot(in), mh = __ballot(head);
    if ((threadIdx.x & 63) == 0) {
        if (mi) atomicAdd(&cnt[PF_PHASED], (ull)__popcll(mi));
        if (mh) atomicAdd(&cnt[PF_BLOCKS], (ull)__popcll(mh));
    }
}

namespace {

struct pf_work {
    unsigned *lp, *hook;
    ull *best, *cnt;
    int *low, *size;
    size_t lay(void *base, size_t ns) {
        tdt_carver cv(base);
        lp = cv.take<unsigned>(ns), hook = cv.take<unsigned>(ns), best = cv.take<ull>(ns), low = cv.take<int>(ns), size = cv.take<int>(ns);
        cnt = cv.take<ull>(PF_CNT_N);
        return cv.size;
    }
};

struct pf_res {                               // the results as one allocation
    pf_out O;
    size_t lay(void *base, size_t ns, size_t nl) {
        tdt_carver cv(base);
        O.root = cv.take<int32_t>(ns), O.phase = cv.take<uint8_t>(ns), O.used = cv.take<uint8_t>(nl ? nl : 1);
        O.agree = cv.take<uint32_t>(ns), O.conflict = cv.take<uint32_t>(ns);
        return cv.size;
    }
};

inline unsigned pf_grid(size_t n) { return (unsigned)((n + PF_BLOCK - 1) / PF_BLOCK); }

// The forest of the link rows (device pointers; ns >= 1, ns < 2^31, nl < 2^31) into O; cnt_out[PF_CNT_N] = the counters, [PF_HOOKS]
// replaced by the rounds run.  `who` names the entry in error texts.  The stream is synchronised.
int pf_run(tdt_ctx *ctx, const char *who, const ull *ji, const unsigned *N, const unsigned *T, size_t nl_, size_t ns_, unsigned S, const pf_out &O, ull *cnt_out) {
    hipStream_t st = ctx->stream;
    const int ns = (int)ns_, nl = (int)nl_;
    void *d_work = nullptr;
    pf_work W;
    const size_t bytes = W.lay(nullptr, ns_);
    if (tdt_dev_malloc(&d_work, bytes) != hipSuccess) {
        tdt_set_error("%s: out of device memory (%zu sites)", who, ns_);
        return TDT_E_NOMEM;
    }
    W.lay(d_work, ns_);
    ull rounds = 0;
    auto body = [&]() -> int {
        ull host[PF_CNT_N];
        TDT_HIP(hipMemsetAsync(W.cnt, 0, PF_CNT_N * 8, st));
        TDT_HIP(hipMemsetAsync(W.best, 0, ns_ * 8, st));
        TDT_HIP(hipMemsetAsync(O.agree, 0, ns_ * 4, st));
        TDT_HIP(hipMemsetAsync(O.conflict, 0, ns_ * 4, st));
        if (nl) TDT_HIP(hipMemsetAsync(O.used, 0, nl_, st));
        hipLaunchKernelGGL(pf_init, dim3(pf_grid(ns_)), dim3(PF_BLOCK), 0, st, ns, W.lp, W.hook, W.low, W.size);
        TDT_CHECK_LAUNCH();
        for (; nl;) {
            if (rounds >= PF_MAX_ROUNDS) {
                tdt_set_error("%s: the forest did not close in %d rounds", who, PF_MAX_ROUNDS);
                return TDT_E_INEXACT;
            }
            TDT_HIP(hipMemsetAsync(W.cnt + PF_HOOKS, 0, 8, st));
            hipLaunchKernelGGL(pf_pick, dim3(pf_grid(nl_)), dim3(PF_BLOCK), 0, st, ji, N, T, nl, S, (const unsigned *)W.lp, W.best);
            TDT_CHECK_LAUNCH();
            hipLaunchKernelGGL(pf_hook, dim3(pf_grid(ns_)), dim3(PF_BLOCK), 0, st, ji, N, T, ns, S, (const unsigned *)W.lp, (const ull *)W.best, W.hook, O.used,
                               W.cnt);
            TDT_CHECK_LAUNCH();
            hipLaunchKernelGGL(pf_apply, dim3(pf_grid(ns_)), dim3(PF_BLOCK), 0, st, ns, W.lp, W.hook, W.best);
            TDT_CHECK_LAUNCH();
            TDT_HIP(hipMemcpyAsync(host, W.cnt, 8, hipMemcpyDeviceToHost, st));
            TDT_HIP(hipStreamSynchronize(st));
            if (!host[PF_HOOKS]) break;
            rounds++;
            cnt_out[PF_EDGES] += host[PF_HOOKS];
            for (int jumps = 0;; jumps++) {                        // (a launch halves every path: 31 launches flatten any)
                if (jumps >= PF_MAX_ROUNDS) {
                    tdt_set_error("%s: the labels did not flatten in %d launches", who, PF_MAX_ROUNDS);
                    return TDT_E_INEXACT;
                }
                TDT_HIP(hipMemsetAsync(W.cnt + PF_CHANGED, 0, 8, st));
                hipLaunchKernelGGL(pf_jump, dim3(pf_grid(ns_)), dim3(PF_BLOCK), 0, st, ns, W.lp, W.cnt);
                TDT_CHECK_LAUNCH();
                TDT_HIP(hipMemcpyAsync(host, W.cnt + PF_CHANGED, 8, hipMemcpyDeviceToHost, st));
                TDT_HIP(hipStreamSynchronize(st));
                if (!host[0]) break;
            }
        }
        hipLaunchKernelGGL(pf_low, dim3(pf_grid(ns_)), dim3(PF_BLOCK), 0, st, ns, (const unsigned *)W.lp, W.low, W.size);
        TDT_CHECK_LAUNCH();
        if (nl) {
            hipLaunchKernelGGL(pf_check, dim3(pf_grid(nl_)), dim3(PF_BLOCK), 0, st, ji, N, T, nl, S, (const unsigned *)W.lp, (const uint8_t *)O.used,
                               (const int *)W.low, O.agree, O.conflict, W.cnt);
            TDT_CHECK_LAUNCH();
        }
        hipLaunchKernelGGL(pf_sites, dim3(pf_grid(ns_)), dim3(PF_BLOCK), 0, st, ns, (const unsigned *)W.lp, (const int *)W.low, (const int *)W.size, O.root,
                           O.phase, W.cnt);
        TDT_CHECK_LAUNCH();
        TDT_HIP(hipMemcpyAsync(host, W.cnt, PF_CNT_N * 8, hipMemcpyDeviceToHost, st));
        TDT_HIP(hipStreamSynchronize(st));
        const ull edges = cnt_out[PF_EDGES];
        memcpy(cnt_out, host, sizeof host);
        cnt_out[PF_EDGES] = edges;
        cnt_out[PF_HOOKS] = rounds;
        return TDT_OK;
    };
    cnt_out[PF_EDGES] = 0;
    const int rc = body();
    (void)hipStreamSynchronize(st);
    (void)hipFree(d_work);
    return rc;
}

// what both generic entries refuse in front of any work
int pf_check_args(const char *who, tdt_ctx *ctx, bool ptrs, size_t nl, size_t ns, uint64_t S) {
    if (!ctx || !ptrs) {
        tdt_set_error("%s: bad argument", who);
        return TDT_E_ARG;
    }
    if (ns >= (1ull << 31) || nl >= (1ull << 31) || S < 1 || S > 0x7fffffffull) {
        tdt_set_error("%s: %zu sites, %zu links (fewer than 2^31 each), min_link %llu (1 ... 2^31 - 1)", who, ns, nl, (ull)S);
        return TDT_E_RANGE;
    }
    return TDT_OK;
}

// the generic entry on device columns: packs the rows (refusing a bad one), then the forest into O
int pf_columns(tdt_ctx *ctx, const char *who, const int32_t *j, const int32_t *i, const uint32_t *N, const uint32_t *T, size_t nl, size_t ns, unsigned S,
               const pf_out &O) {
    if (!ns) return TDT_OK;
    hipStream_t st = ctx->stream;
    ull *ji = nullptr, *flag = nullptr;
    if (tdt_dev_malloc((void **)&ji, (nl + 1) * 8 + 256) != hipSuccess) {
        tdt_set_error("%s: out of device memory (%zu links)", who, nl);
        return TDT_E_NOMEM;
    }
    flag = ji + nl + 1;
    auto body = [&]() -> int {
        ull host[PF_CNT_N] = {};
        if (nl) {
            TDT_HIP(hipMemsetAsync(flag, 0, 8, st));
            hipLaunchKernelGGL(pf_pack, dim3(pf_grid(nl)), dim3(PF_BLOCK), 0, st, j, i, N, T, (int)nl, (int)ns, ji, flag);
            TDT_CHECK_LAUNCH();
            TDT_HIP(hipMemcpyAsync(host, flag, 8, hipMemcpyDeviceToHost, st));
            TDT_HIP(hipStreamSynchronize(st));
            if (host[0]) {
                tdt_set_error("%s: a link row with an end outside [0, %zu), two equal ends, or TRANS > N", who, ns);
                return TDT_E_ARG;
            }
        }
        return pf_run(ctx, who, ji, N, T, nl, ns, S, O, host);
    };
    const int rc = body();
    (void)hipStreamSynchronize(st);
    (void)hipFree(ji);
    return rc;
}

}  // namespace

extern "C" int tdt_phase_forest_device(tdt_ctx *ctx, const int32_t *d_j, const int32_t *d_i, const uint32_t *d_n, const uint32_t *d_trans, size_t n_links,
                                       size_t n_sites, uint64_t min_link, int32_t *d_root, uint8_t *d_phase, uint8_t *d_edge_used, uint32_t *d_agree,
                                       uint32_t *d_conflict) {
    const bool ptrs = (!n_links || (d_j && d_i && d_n && d_trans && d_edge_used)) && (!n_sites || (d_root && d_phase && d_agree && d_conflict));
    const int rc = pf_check_args("tdt_phase_forest_device", ctx, ptrs, n_links, n_sites, min_link);
    if (rc) return rc;
    TDT_HIP(hipSetDevice(ctx->device));
    return pf_columns(ctx, "tdt_phase_forest_device", d_j, d_i, d_n, d_trans, n_links, n_sites, (unsigned)min_link,
                      pf_out{d_root, d_phase, d_edge_used, d_agree, d_conflict});
}

extern "C" int tdt_phase_forest(tdt_ctx *ctx, const int32_t *j, const int32_t *i, const uint32_t *n, const uint32_t *trans, size_t n_links, size_t n_sites,
                                uint64_t min_link, int32_t *root, uint8_t *phase, uint8_t *edge_used, uint32_t *agree, uint32_t *conflict) {
    const bool ptrs = (!n_links || (j && i && n && trans && edge_used)) && (!n_sites || (root && phase && agree && conflict));
    int rc = pf_check_args("tdt_phase_forest", ctx, ptrs, n_links, n_sites, min_link);
    if (rc) return rc;
    if (!n_sites) return TDT_OK;
    TDT_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    struct in_lay {
        int32_t *j, *i;
        uint32_t *n, *t;
        size_t lay(void *base, size_t nl) {
            tdt_carver cv(base);
            j = cv.take<int32_t>(nl), i = cv.take<int32_t>(nl), n = cv.take<uint32_t>(nl), t = cv.take<uint32_t>(nl);
            return cv.size;
        }
    } In;
    pf_res Res;
    void *d_in = nullptr, *d_res = nullptr;
    if (tdt_dev_malloc(&d_in, In.lay(nullptr, n_links) + 256) != hipSuccess || tdt_dev_malloc(&d_res, Res.lay(nullptr, n_sites, n_links)) != hipSuccess) {
        if (d_in) (void)hipFree(d_in);
        tdt_set_error("tdt_phase_forest: out of device memory (%zu sites, %zu links)", n_sites, n_links);
        return TDT_E_NOMEM;
    }
    In.lay(d_in, n_links);
    Res.lay(d_res, n_sites, n_links);
    auto body = [&]() -> int {
        if (n_links) {
            TDT_HIP(hipMemcpyAsync(In.j, j, n_links * 4, hipMemcpyHostToDevice, st));
            TDT_HIP(hipMemcpyAsync(In.i, i, n_links * 4, hipMemcpyHostToDevice, st));
            TDT_HIP(hipMemcpyAsync(In.n, n, n_links * 4, hipMemcpyHostToDevice, st));
            TDT_HIP(hipMemcpyAsync(In.t, trans, n_links * 4, hipMemcpyHostToDevice, st));
        }
        const int rc2 = pf_columns(ctx, "tdt_phase_forest", In.j, In.i, In.n, In.t, n_links, n_sites, (unsigned)min_link, Res.O);
        if (rc2) return rc2;
        TDT_HIP(hipMemcpyAsync(root, Res.O.root, n_sites * 4, hipMemcpyDeviceToHost, st));
        TDT_HIP(hipMemcpyAsync(phase, Res.O.phase, n_sites, hipMemcpyDeviceToHost, st));
        TDT_HIP(hipMemcpyAsync(agree, Res.O.agree, n_sites * 4, hipMemcpyDeviceToHost, st));
        TDT_HIP(hipMemcpyAsync(conflict, Res.O.conflict, n_sites * 4, hipMemcpyDeviceToHost, st));
        if (n_links) TDT_HIP(hipMemcpyAsync(edge_used, Res.O.used, n_links, hipMemcpyDeviceToHost, st));
        TDT_HIP(hipStreamSynchronize(st));
        return TDT_OK;
    };
    rc = body();
    (void)hipStreamSynchronize(st);
    (void)hipFree(d_in);
    (void)hipFree(d_res);
    return rc;
}

// ---- the phase state of an allele handle
void tdt_phase_free(tdt_phase *p) {
    if (!p) return;
    (void)hipSetDevice(p->ctx->device);
    (void)hipStreamSynchronize(p->ctx->stream);
    ks_free(&p->S);
    ks_free(&p->L);
    if (p->d_codes) (void)hipFree(p->d_codes);
    if (p->d_het) (void)hipFree(p->d_het);
    if (p->d_res) (void)hipFree(p->d_res);
    delete p;
}

int tdt_phase_create(tdt_ctx *ctx, const int32_t *d_pos, const long long *d_off, size_t ns, int n_contigs, int min_q, int min_bq, const uint8_t *site_codes,
                     size_t capacity, int hash_bits, tdt_phase **out) {
    if (hash_bits < 1 || hash_bits > 64 || min_q < 0 || min_q > 255 || n_contigs > KS_MAX_CONTIGS || capacity >= (1ull << 40)) {
        tdt_set_error("tdt_alleles_phase_enable: hash_bits %d (1 ... 64), min_q %d (0 ... 255), %d contigs (at most 2^24), capacity %zu", hash_bits, min_q,
                      n_contigs, capacity);
        return TDT_E_RANGE;
    }
    for (size_t k = 0; k < ns; k++) {
        const unsigned c = site_codes[k];
        if (c != 0xffu && (c > 15u || (c & 3u) == (c >> 2))) {
            tdt_set_error("tdt_alleles_phase_enable: site %zu: code %u is neither ref2 | alt2 << 2 of two different bases nor 0xff", k, c);
            return TDT_E_ARG;
        }
    }
    tdt_phase *p = new tdt_phase{};
    p->ctx = ctx;
    p->ns = ns;
    p->min_q = min_q, p->min_bq = min_bq;
    p->hash_mask = hash_bits == 64 ? ~0ull : (1ull << hash_bits) - 1ull;
    hipStream_t st = ctx->stream;
    auto body = [&]() -> int {
        const size_t N = ns ? ns : 1;
        if (tdt_dev_malloc((void **)&p->d_codes, N) != hipSuccess || tdt_dev_malloc((void **)&p->d_het, N) != hipSuccess) {
            tdt_set_error("tdt_alleles_phase_enable: out of device memory (%zu sites)", ns);
            return TDT_E_NOMEM;
        }
        int rc = ks_init(&p->S, ctx, "tdt_alleles_phase", PK_OR1, capacity);
        if (rc == TDT_OK) rc = ks_init(&p->L, ctx, "tdt_alleles_phase_links", LK_OR1, 0);
        if (rc) return rc;
        if (ns) TDT_HIP(hipMemcpyAsync(p->d_codes, site_codes, ns, hipMemcpyHostToDevice, st));
        TDT_HIP(hipStreamSynchronize(st));
        return TDT_OK;
    };
    const int rc = body();
    if (rc) {
        tdt_phase_free(p);
        return rc;
    }
    p->T = ph_table{d_pos, d_off, p->d_codes, n_contigs};
    *out = p;
    return TDT_OK;
}

int tdt_phase_reset(tdt_phase *p) {
    p->done = false;
    const int rc = ks_reset(&p->S);
    return rc ? rc : ks_reset(&p->L);
}

// PH_MAX_OBS slots of the store per read, the bound a read's cap gives (ks_launch reserves them BEFORE the launch)
int tdt_phase_push(tdt_phase *p, const tdt_batch &B, size_t n, size_t raw_len) {
    p->done = false;
    return ks_launch(&p->S, n * PH_MAX_OBS, [&] {
        hipLaunchKernelGGL(phase_keys, dim3((unsigned)((n + PH_BLOCK - 1) / PH_BLOCK)), dim3(PH_BLOCK), 0, p->ctx->stream, ks_cols_of(B), B.end, (int)n, (ull)raw_len,
                           (unsigned)p->min_q, p->min_bq, p->T, p->hash_mask, p->S.k1, p->S.k2, (ull)p->S.cap, p->S.d_state);
    });
}

static tdt_phase *ph_of(tdt_alleles *h, const char *fn, bool ok = true) {
    tdt_phase *p = tdt_alleles_phase_of(h);
    if (!p || !ok) {
        tdt_set_error("%s: bad argument, or no tdt_alleles_phase_enable", fn);
        return nullptr;
    }
    return p;
}

// The observation store read out, in the order it lies in HBM (ks_keys' convention for *n)
extern "C" int tdt_alleles_phase_keys(tdt_alleles *h, uint64_t *k1, uint64_t *k2, size_t *n) {
    tdt_phase *p = ph_of(h, "tdt_alleles_phase_keys");
    return p ? ks_keys(&p->S, "tdt_alleles_phase", k1, k2, n) : TDT_E_ARG;
}

static double ph_ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// The finish (see the head of this file).  het_flags: HOST, one byte per device site.  got[TDT_PHASE_GOT_N]: the four push counters, then
// fragment_rows discordant_rows cross_contig_pairs links weak_links forest_edges agree conflict phased_sites blocks, and the rounds run.
// The stores are left as they were: a later push goes on, a second finish gives the same.
extern "C" int tdt_alleles_phase_finish(tdt_alleles *h, const uint8_t *het_flags, uint64_t min_link, uint64_t *got) {
    tdt_phase *p = tdt_alleles_phase_of(h);
    p = ph_of(h, "tdt_alleles_phase_finish", got && (het_flags || (p && !p->ns)));
    if (!p) return TDT_E_ARG;
    if (min_link < 1 || min_link > 0x7fffffffull) {
        tdt_set_error("tdt_alleles_phase_finish: min_link %llu (1 ... 2^31 - 1)", (ull)min_link);
        return TDT_E_RANGE;
    }
    tdt_ctx *ctx = p->ctx;
    TDT_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    p->done = false;
    uint64_t res[TDT_PHASE_GOT_N] = {};
    for (int k = 0; k < 5; k++) p->ms[k] = 0;
    // 1: the fragment rows
    auto t0 = std::chrono::steady_clock::now();
    ull state[KS_WORDS], g2[2];
    int rc = ks_stored(&p->S, state);
    if (rc == TDT_OK) rc = ks_finish(&p->S, state, 1, g2);
    if (rc) return rc;
    for (int k = 0; k < PK_N; k++) res[k] = state[k];
    const size_t nrows = p->S.n_rows;
    res[PK_N] = nrows;
    p->ms[0] = ph_ms_since(t0);
    // 2: the link keys into the second store
    t0 = std::chrono::steady_clock::now();
    rc = ks_reset(&p->L);
    if (rc) return rc;
    if (p->ns) TDT_HIP(hipMemcpyAsync(p->d_het, het_flags, p->ns, hipMemcpyHostToDevice, st));
    if (nrows) {
        rc = ks_launch(&p->L, nrows, [&] {
            hipLaunchKernelGGL(phase_links, dim3((unsigned)((nrows + PHL_TILE - 1) / PHL_TILE)), dim3(PHL_TILE), 0, st, (const ull *)p->S.r_k1, (const ull *)p->S.r_k2,
                               (const unsigned *)p->S.r_sup, (const unsigned *)p->S.r_rev, (int)nrows, (const uint8_t *)p->d_het, p->T.off, p->T.n_contigs, p->L.k1,
                               p->L.k2, (ull)p->L.cap, p->L.d_state);
        });
        if (rc) return rc;
    }
    rc = ks_stored(&p->L, state);                                   // (synchronises: het_flags is free again)
    if (rc) return rc;
    res[PK_N + 1] = state[LK_DISCORDANT], res[PK_N + 2] = state[LK_CROSS];
    p->ms[1] = ph_ms_since(t0);
    // 3: the link rows
    t0 = std::chrono::steady_clock::now();
    rc = ks_finish(&p->L, state, 1, g2);
    if (rc) return rc;
    const size_t nl = p->L.n_rows;
    res[PK_N + 3] = nl;
    p->n_links = nl;
    p->ms[2] = ph_ms_since(t0);
    // 4 - 6: the forest, the check, the sites
    t0 = std::chrono::steady_clock::now();
    if (p->ns) {
        pf_res Res;
        const size_t bytes = Res.lay(nullptr, p->ns, nl);
        if (bytes > p->res_cap) {
            if (p->d_res) TDT_HIP(hipFree(p->d_res));
            p->d_res = nullptr, p->res_cap = 0;
            if (tdt_dev_malloc(&p->d_res, bytes) != hipSuccess) {
                tdt_set_error("tdt_alleles_phase_finish: out of device memory (%zu sites, %zu links)", p->ns, nl);
                return TDT_E_NOMEM;
            }
            p->res_cap = bytes;
        }
        Res.lay(p->d_res, p->ns, nl);
        p->R = Res.O;
        ull cnt[PF_CNT_N] = {};
        rc = pf_run(ctx, "tdt_alleles_phase_finish", (const ull *)p->L.r_k1, (const unsigned *)p->L.r_sup, (const unsigned *)p->L.r_rev, nl, p->ns, (unsigned)min_link,
                    p->R, cnt);
        if (rc) return rc;
        uint64_t *r = res + PK_N + 4;
        r[0] = cnt[PF_WEAK], r[1] = cnt[PF_EDGES], r[2] = cnt[PF_AGREE], r[3] = cnt[PF_CONFLICT], r[4] = cnt[PF_PHASED], r[5] = cnt[PF_BLOCKS], r[6] = cnt[PF_HOOKS];
    }
    p->ms[3] = ph_ms_since(t0);
    memcpy(got, res, sizeof res);
    p->done = true;
    return TDT_OK;
}

static tdt_phase *ph_done(tdt_alleles *h, const char *fn, bool ok) {
    tdt_phase *p = ph_of(h, fn, ok);
    if (p && !p->done) {
        tdt_set_error("%s: no tdt_alleles_phase_finish since the last push or reset", fn);
        return nullptr;
    }
    return p;
}

// per device site of the last finish: root = the global index of its block's lowest site (-1: in no block), phase = 0 / 1 against that site
extern "C" int tdt_alleles_phase_sites(tdt_alleles *h, int32_t *root, uint8_t *phase, size_t n) {
    tdt_phase *p = ph_done(h, "tdt_alleles_phase_sites", tdt_alleles_phase_of(h) && n == tdt_alleles_phase_of(h)->ns && (!n || (root && phase)));
    if (!p) return TDT_E_ARG;
    if (!n) return TDT_OK;
    TDT_HIP(hipSetDevice(p->ctx->device));
    hipStream_t st = p->ctx->stream;
    TDT_HIP(hipMemcpyAsync(root, p->R.root, n * 4, hipMemcpyDeviceToHost, st));
    TDT_HIP(hipMemcpyAsync(phase, p->R.phase, n, hipMemcpyDeviceToHost, st));
    TDT_HIP(hipStreamSynchronize(st));
    return TDT_OK;
}

// the blocks of the last finish, ascending: first and last site (global indices), sites, eligible links (sites - 1 forest edges + agree +
// conflict), agree, conflict.  *n in: the room of the six arrays (ignored when all are NULL), out: the blocks
extern "C" int tdt_alleles_phase_blocks(tdt_alleles *h, int32_t *start, int32_t *end, uint32_t *sites, uint32_t *edges, uint32_t *agree, uint32_t *conflict, size_t *n) {
    const bool any = start || end || sites || edges || agree || conflict;
    tdt_phase *p = ph_done(h, "tdt_alleles_phase_blocks", n && (!any || (start && end && sites && edges && agree && conflict)));
    if (!p) return TDT_E_ARG;
    const size_t ns = p->ns;
    std::vector<int32_t> root(ns);
    std::vector<uint32_t> ag(ns), co(ns), slot(ns), size;
    std::vector<int32_t> first, last;
    if (ns) {
        TDT_HIP(hipSetDevice(p->ctx->device));
        hipStream_t st = p->ctx->stream;
        TDT_HIP(hipMemcpyAsync(root.data(), p->R.root, ns * 4, hipMemcpyDeviceToHost, st));
        TDT_HIP(hipMemcpyAsync(ag.data(), p->R.agree, ns * 4, hipMemcpyDeviceToHost, st));
        TDT_HIP(hipMemcpyAsync(co.data(), p->R.conflict, ns * 4, hipMemcpyDeviceToHost, st));
        TDT_HIP(hipStreamSynchronize(st));
    }
    for (size_t v = 0; v < ns; v++) {                               // (a block's lowest site comes first: its slot exists when a later site names it)
        const int32_t r = root[v];
        if (r < 0) continue;
        if ((size_t)r == v) {
            slot[v] = (uint32_t)first.size();
            first.push_back(r), last.push_back(r), size.push_back(0);
        }
        const uint32_t b = slot[(size_t)r];
        size[b]++;
        last[b] = (int32_t)v;
    }
    const size_t have = first.size();
    if (any) {
        if (*n < have) {
            tdt_set_error("tdt_alleles_phase_blocks: room for %zu blocks, %zu found", *n, have);
            return TDT_E_RANGE;
        }
        for (size_t b = 0; b < have; b++) {
            const size_t v = (size_t)first[b];
            start[b] = first[b], end[b] = last[b], sites[b] = size[b], agree[b] = ag[v], conflict[b] = co[v];
            edges[b] = size[b] - 1 + ag[v] + co[v];
        }
    }
    *n = have;
    return TDT_OK;
}

// the link rows of the last finish, ascending by (j, i): the two sites (global indices, i < j), N and TRANS, and whether the link is a
// forest edge.  *n as above
extern "C" int tdt_alleles_phase_links(tdt_alleles *h, uint32_t *j, uint32_t *i, uint32_t *n_, uint32_t *trans, uint8_t *edge_used, size_t *n) {
    const bool any = j || i || n_ || trans || edge_used;
    tdt_phase *p = ph_done(h, "tdt_alleles_phase_links", n && (!any || (j && i && n_ && trans && edge_used)));
    if (!p) return TDT_E_ARG;
    const size_t have = p->n_links;
    if (any) {
        if (*n < have) {
            tdt_set_error("tdt_alleles_phase_links: room for %zu links, %zu found", *n, have);
            return TDT_E_RANGE;
        }
        if (have) {
            std::vector<uint64_t> ji(have);
            TDT_HIP(hipSetDevice(p->ctx->device));
            hipStream_t st = p->ctx->stream;
            TDT_HIP(hipMemcpyAsync(ji.data(), p->L.r_k1, have * 8, hipMemcpyDeviceToHost, st));
            TDT_HIP(hipMemcpyAsync(n_, p->L.r_sup, have * 4, hipMemcpyDeviceToHost, st));
            TDT_HIP(hipMemcpyAsync(trans, p->L.r_rev, have * 4, hipMemcpyDeviceToHost, st));
            if (p->ns) TDT_HIP(hipMemcpyAsync(edge_used, p->R.used, have, hipMemcpyDeviceToHost, st));
            TDT_HIP(hipStreamSynchronize(st));
            for (size_t x = 0; x < have; x++) j[x] = (uint32_t)(ji[x] >> 32), i[x] = (uint32_t)ji[x];
        }
    }
    *n = have;
    return TDT_OK;
}

// host milliseconds of the last finish's launch groups, each ended by a synchronisation: [0] the observation store's finish, [1] phase_links
// and its counters, [2] the link store's finish, [3] the forest, the check and the sites; [4] = device milliseconds of [0]'s and [2]'s sorts
extern "C" int tdt_alleles_phase_timing(tdt_alleles *h, double *ms5) {
    tdt_phase *p = ph_of(h, "tdt_alleles_phase_timing", ms5 != nullptr);
    if (!p) return TDT_E_ARG;
    for (int k = 0; k < 4; k++) ms5[k] = p->ms[k];
    ms5[4] = p->S.ms[0] + p->S.ms[2] + p->L.ms[0] + p->L.ms[2];
    return TDT_OK;
}

// out3 of the observation store: asks of the device for the real count, growths, the capacity now
extern "C" int tdt_alleles_phase_reserve_stats(tdt_alleles *h, uint64_t *out3) {
    tdt_phase *p = ph_of(h, "tdt_alleles_phase_reserve_stats", out3 != nullptr);
    return p ? ks_reserve_stats(&p->S, "tdt_alleles_phase", out3) : TDT_E_ARG;
}
