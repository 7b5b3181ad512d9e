/* What ntl_pairtab_create (ntl_hip.hip) reads of a tally (ntl_pairs.cpp), so that the name ranks, k and f have one definition: the
 * arrays are the tally's own and live as long as it does.  Not part of the C ABI. */
#pragma once
#include <stdint.h>

struct ntl_tally;
struct TallyView { const uint32_t *rank, *ctg_len; uint64_t n_ctg; int k, f; };
TallyView ntl_tally_view(const ntl_tally *t);
