/* verify_digests.c - a plain C caller of ed25519_verify_digests and ed25519_verify_digests_rlc (include/eddsa_amd.h) against the
 * SHIPPED library:  verify_digests sigs.bin pubs.bin digests.bin want.bin
 * The four files hold n packed items (64, 32, 64 and 1 byte each); tests/test_gpu_digests.py writes them, with the expected
 * verdicts from the oracle.  Exit status 0 and "verify_digests: ok" when both calls return exactly those verdicts. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "eddsa_amd.h"

static uint8_t *slurp(const char *path, size_t *len)
{
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    fseek(f, 0, SEEK_END);
    long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t *buf = malloc(sz > 0 ? (size_t)sz : 1);
    if (!buf || fread(buf, 1, (size_t)sz, f) != (size_t)sz) { fprintf(stderr, "%s: short read\n", path); exit(2); }
    fclose(f);
    *len = (size_t)sz;
    return buf;
}

static int same(const char *what, const uint8_t *got, const uint8_t *want, size_t n)
{
    for (size_t i = 0; i < n; i++)
        if (got[i] != want[i]) { fprintf(stderr, "%s: item %zu: verdict %d, expected %d\n", what, i, got[i], want[i]); return 0; }
    return 1;
}

int main(int argc, char **argv)
{
    if (argc != 5) { fprintf(stderr, "usage: %s sigs pubs digests want\n", argv[0]); return 2; }
    size_t ls, lp, ld, n;
    uint8_t *sigs = slurp(argv[1], &ls), *pubs = slurp(argv[2], &lp), *digests = slurp(argv[3], &ld), *want = slurp(argv[4], &n);
    if (ls != 64 * n || lp != 32 * n || ld != 64 * n || n == 0) { fprintf(stderr, "the files disagree on the number of items\n"); return 2; }
    uint8_t *ok = malloc(n);
    uint32_t stats[4];
    int rc;

    memset(ok, 0xee, n);
    if ((rc = ed25519_verify_digests(ok, sigs, pubs, digests, n)) != 0) { fprintf(stderr, "ed25519_verify_digests: %s\n", eddsa_amd_strerror(rc)); return 1; }
    if (!same("ed25519_verify_digests", ok, want, n)) return 1;

    /* a call this small goes to the per-item kernels by default: every item is counted as decided per item */
    memset(ok, 0xee, n);
    if ((rc = ed25519_verify_digests_rlc(ok, stats, sigs, pubs, digests, n)) != 0) { fprintf(stderr, "ed25519_verify_digests_rlc: %s\n", eddsa_amd_strerror(rc)); return 1; }
    if (!same("ed25519_verify_digests_rlc", ok, want, n)) return 1;
    if (stats[0] != 0 || stats[1] != n || stats[3] != 0) { fprintf(stderr, "rlc statistics below the threshold: %u %u %u %u\n", stats[0], stats[1], stats[2], stats[3]); return 1; }

    /* and through the combination itself: the groups that do not pass fall back to the per-item kernels */
    eddsa_amd_set_rlc_min_items(0);
    memset(ok, 0xee, n);
    rc = ed25519_verify_digests_rlc(ok, stats, sigs, pubs, digests, n);
    eddsa_amd_set_rlc_min_items(EDDSA_AMD_RLC_MIN_ITEMS_DEFAULT);
    if (rc != 0) { fprintf(stderr, "ed25519_verify_digests_rlc (combining): %s\n", eddsa_amd_strerror(rc)); return 1; }
    if (!same("ed25519_verify_digests_rlc (combining)", ok, want, n)) return 1;
    if (stats[0] + stats[1] != n) { fprintf(stderr, "rlc statistics: %u + %u items of %zu\n", stats[0], stats[1], n); return 1; }

    eddsa_amd_shutdown();
    printf("verify_digests: ok (%zu items)\n", n);
    free(ok); free(sigs); free(pubs); free(digests); free(want);
    return 0;
}
