/* field_hook.c -- the reference encoder with its motion search replaced, for one picture at a time, by a field the test chose.
 *
 * oracle/Makefile links this file with the reference's sources into _ref/libdsv2ref_field.so; hme.c alone is compiled with
 * -Ddsv_hme=dsv2ref_searched_hme, so the dsv_hme that motion_est (dsv_encoder.c:679) calls is the one below.  With nothing
 * queued it is the reference's search and the library codes what libdsv2ref.so codes (tests/test_field_cases_ref.py).
 * With a field queued, that field becomes hme->mvf[0] -- allocated with the reference's allocator, since the encoder frees it
 * -- and the three results motion_est expects are derived from four integers exactly as hme.c derives them from its own
 * sums: intra_pct = nintra * 100 / nb (hme.c:2015), scblocks = ndiff * 100 / max(eligible, 1) (hme.c:1825-1829),
 * avg_err = total_err / nb (hme.c:1830).  Test infrastructure only, never preloaded: tests dlopen it. */
#include <string.h>

#include "dsv_encoder.h"
#include "dsv_internal.h"

extern int dsv2ref_searched_hme(DSV_HME *hme, int *scene_change_blocks, int *avg_err);

static DSV_MV *pending;
static int pending_n, pending_ints[4];

/* queue `field` (nblocks records, copied) for the next picture this process searches; field == NULL drops a queued one.
 * Returns 0, or -1 for a bad argument. */
int dsv2ref_set_field(const DSV_MV *field, int nblocks, int nintra, int ndiff, int eligible, unsigned total_err)
{
    if (pending) {
        dsv_free(pending);
        pending = NULL;
    }
    if (!field) {
        return 0;
    }
    if (nblocks <= 0) {
        return -1;
    }
    pending = dsv_alloc((int) sizeof(DSV_MV) * nblocks);
    memcpy(pending, field, sizeof(DSV_MV) * (size_t) nblocks);
    pending_n = nblocks;
    pending_ints[0] = nintra;
    pending_ints[1] = ndiff;
    pending_ints[2] = eligible;
    pending_ints[3] = (int) total_err;
    return 0;
}

int dsv_hme(DSV_HME *hme, int *scene_change_blocks, int *avg_err)
{
    const int nb = hme->params->nblocks_h * hme->params->nblocks_v;
    if (!pending) {
        return dsv2ref_searched_hme(hme, scene_change_blocks, avg_err);
    }
    if (pending_n != nb) { /* a field for another geometry: drop it, search */
        dsv_free(pending);
        pending = NULL;
        return dsv2ref_searched_hme(hme, scene_change_blocks, avg_err);
    }
    hme->mvf[0] = pending; /* (levels 1.. stay NULL: motion_est frees only what is there) */
    pending = NULL;
    *scene_change_blocks = pending_ints[1] * 100 / (pending_ints[2] ? pending_ints[2] : 1);
    *avg_err = (int) ((unsigned) pending_ints[3] / (unsigned) nb);
    return pending_ints[0] * 100 / nb;
}
