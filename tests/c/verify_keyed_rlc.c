/* verify_keyed_rlc.c - a plain C caller of the batch verification over a key set (include/eddsa_amd.h: ed25519_verify_keyed_rlc)
 * against the SHIPPED library:  verify_keyed_rlc keys.bin idx.bin sigs.bin msgs.bin want.bin combined
 * keys: 32 bytes per key; idx, sigs, msgs (32 bytes each), want: 4, 64, 32 and 1 byte per item; combined: the number of items the
 * combination is expected to decide; tests/test_gpu_keyed_rlc.py writes them, with the expected verdicts from the oracle.
 * Exit status 0 and "verify_keyed_rlc: ok" when every call returns those. */
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
    if (argc != 7) { fprintf(stderr, "usage: %s keys idx sigs msgs want combined\n", argv[0]); return 2; }
    size_t lk, li, ls, lm, n;
    uint8_t *keys = slurp(argv[1], &lk), *idx = slurp(argv[2], &li), *sigs = slurp(argv[3], &ls), *msgs = slurp(argv[4], &lm),
            *want = slurp(argv[5], &n);
    const uint32_t combined = (uint32_t)strtoul(argv[6], NULL, 10);
    if (lk == 0 || lk % 32 || li != 4 * n || ls != 64 * n || lm != 32 * n || n == 0) { fprintf(stderr, "the files disagree on the number of items\n"); return 2; }
    const size_t count = lk / 32;
    uint8_t *ok = malloc(n);
    uint32_t stats[4] = { 9, 9, 9, 9 };
    eddsa_amd_keyset *ks = NULL;
    int rc;

    if (ed25519_verify_keyed_rlc(ok, stats, NULL, (const uint32_t *)idx, sigs, msgs, NULL, 32, n) == 0) { fprintf(stderr, "no key set accepted\n"); return 1; }
    if ((rc = eddsa_amd_keyset_create(&ks, keys, count)) != 0) { fprintf(stderr, "eddsa_amd_keyset_create: %s\n", eddsa_amd_strerror(rc)); return 1; }

    /* every call is combined, whatever its size */
    eddsa_amd_set_rlc_min_items(0);
    memset(ok, 0xee, n);
    if ((rc = ed25519_verify_keyed_rlc(ok, stats, ks, (const uint32_t *)idx, sigs, msgs, NULL, 32, n)) != 0) { fprintf(stderr, "ed25519_verify_keyed_rlc: %s\n", eddsa_amd_strerror(rc)); return 1; }
    if (!same("ed25519_verify_keyed_rlc", ok, want, n)) return 1;
    if (stats[0] != combined || stats[0] + stats[1] != n) { fprintf(stderr, "stats: %u combined, %u per item; expected %u of %zu\n", stats[0], stats[1], combined, n); return 1; }

    /* below the threshold: the keyed per-item kernels, the same verdicts, and the statistics say so */
    eddsa_amd_set_rlc_min_items(n + 1);
    memset(ok, 0xee, n);
    if ((rc = ed25519_verify_keyed_rlc(ok, stats, ks, (const uint32_t *)idx, sigs, msgs, NULL, 32, n)) != 0) { fprintf(stderr, "ed25519_verify_keyed_rlc, per item: %s\n", eddsa_amd_strerror(rc)); return 1; }
    if (!same("ed25519_verify_keyed_rlc, per item", ok, want, n)) return 1;
    if (stats[0] != 0 || stats[1] != n || stats[3] != 0) { fprintf(stderr, "stats of a per-item call: %u %u %u %u\n", stats[0], stats[1], stats[2], stats[3]); return 1; }
    eddsa_amd_set_rlc_min_items(0);

    /* statistics are optional; an empty call touches nothing; a host buffer is no device buffer */
    memset(ok, 0xee, n);
    if ((rc = ed25519_verify_keyed_rlc(ok, NULL, ks, (const uint32_t *)idx, sigs, msgs, NULL, 32, n)) != 0 || !same("without statistics", ok, want, n)) { fprintf(stderr, "stats == NULL\n"); return 1; }
    if (ed25519_verify_keyed_rlc(ok, stats, ks, (const uint32_t *)idx, sigs, msgs, NULL, 32, 0) != 0) { fprintf(stderr, "n = 0\n"); return 1; }
    if (ed25519_verify_keyed_rlc_dev(ok, NULL, ks, (const uint32_t *)idx, sigs, msgs, NULL, 32, n, NULL) == 0) { fprintf(stderr, "a host buffer passed as a device buffer\n"); return 1; }

    eddsa_amd_keyset_destroy(ks);
    eddsa_amd_shutdown();
    printf("verify_keyed_rlc: ok (%zu items, %zu keys, %u combined)\n", n, count, combined);
    free(ok); free(keys); free(idx); free(sigs); free(msgs); free(want);
    return 0;
}
