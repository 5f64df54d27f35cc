// What tdt_alleles.hip and tdt_phase.hip know of each other (TIDDIT_PHASE): the allele handle owns a tdt_phase once
// tdt_alleles_phase_enable has made one, forwards every batch of its two push entries to it, resets and frees it with itself; the phase
// entries of the C ABI reach it through the handle.  The sites (positions, contig offsets) stay the allele handle's: the phase state
// borrows the device pointers for its own lifetime, which ends inside the handle's.
#pragma once
#include "tdt_batch.h"

struct tdt_phase;
struct tdt_alleles;

// d_pos / d_off: the allele handle's device tables (ns sites, n_contigs + 1 offsets); site_codes: HOST, one byte per site
int tdt_phase_create(tdt_ctx *ctx, const int32_t *d_pos, const long long *d_off, size_t ns, int n_contigs, int min_q, int min_bq,
                     const uint8_t *site_codes, size_t capacity, int hash_bits, tdt_phase **out);
// one batch B (device columns, the ones al_count has just read): phase_keys is enqueued on the context's stream
int tdt_phase_push(tdt_phase *p, const tdt_batch &B, size_t n, size_t raw_len);
int tdt_phase_reset(tdt_phase *p);
void tdt_phase_free(tdt_phase *p);
// tdt_alleles.hip: the phase state of a handle (NULL without tdt_alleles_phase_enable, or for a NULL handle)
tdt_phase *tdt_alleles_phase_of(tdt_alleles *h);
