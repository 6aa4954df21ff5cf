/* verify_keyed.c - a plain C caller of the key-set interface (include/eddsa_amd.h: eddsa_amd_keyset_*, ed25519_verify_keyed)
 * against the SHIPPED library:  verify_keyed keys.bin idx.bin sigs.bin msgs.bin want.bin
 * keys: 32 bytes per key; idx, sigs, msgs (32 bytes each), want: 4, 64, 32 and 1 byte per item; tests/test_gpu_keyed.py writes
 * them, with the expected verdicts from the oracle.  Exit status 0 and "verify_keyed: ok" when every call returns those. */
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
    if (argc != 6) { fprintf(stderr, "usage: %s keys idx sigs msgs want\n", argv[0]); return 2; }
    size_t lk, li, ls, lm, n;
    uint8_t *keys = slurp(argv[1], &lk), *idx = slurp(argv[2], &li), *sigs = slurp(argv[3], &ls), *msgs = slurp(argv[4], &lm),
            *want = slurp(argv[5], &n);
    if (lk == 0 || lk % 32 || li != 4 * n || ls != 64 * n || lm != 32 * n || n == 0) { fprintf(stderr, "the files disagree on the number of items\n"); return 2; }
    const size_t count = lk / 32;
    uint8_t *ok = malloc(n);
    eddsa_amd_keyset *ks = (eddsa_amd_keyset *)keys, *none = (eddsa_amd_keyset *)keys;
    int rc;

    /* the argument checks leave *out NULL */
    if (eddsa_amd_keyset_create(&none, keys, 0) == 0 || none != NULL) { fprintf(stderr, "count 0 accepted\n"); return 1; }
    none = (eddsa_amd_keyset *)keys;
    if (eddsa_amd_keyset_create(&none, NULL, count) == 0 || none != NULL) { fprintf(stderr, "keys NULL accepted\n"); return 1; }
    none = (eddsa_amd_keyset *)keys;
    if (eddsa_amd_keyset_create(&none, keys, EDDSA_AMD_KEYSET_MAX_KEYS + 1) == 0 || none != NULL) { fprintf(stderr, "count above the limit accepted\n"); return 1; }

    if ((rc = eddsa_amd_keyset_create(&ks, keys, count)) != 0) { fprintf(stderr, "eddsa_amd_keyset_create: %s\n", eddsa_amd_strerror(rc)); return 1; }
    if (eddsa_amd_keyset_count(ks) != count || eddsa_amd_keyset_device(ks) < 0) { fprintf(stderr, "count / device of the key set\n"); return 1; }
    memset(keys, 0, lk);                             /* the caller's copy is not needed once create has returned */

    memset(ok, 0xee, n);
    if ((rc = ed25519_verify_keyed(ok, ks, (const uint32_t *)idx, sigs, msgs, NULL, 32, n)) != 0) { fprintf(stderr, "ed25519_verify_keyed: %s\n", eddsa_amd_strerror(rc)); return 1; }
    if (!same("ed25519_verify_keyed", ok, want, n)) return 1;

    /* the key set outlives the engines */
    eddsa_amd_shutdown();
    memset(ok, 0xee, n);
    if ((rc = ed25519_verify_keyed(ok, ks, (const uint32_t *)idx, sigs, msgs, NULL, 32, n)) != 0) { fprintf(stderr, "ed25519_verify_keyed after shutdown: %s\n", eddsa_amd_strerror(rc)); return 1; }
    if (!same("ed25519_verify_keyed after shutdown", ok, want, n)) return 1;

    /* an empty call touches nothing; a host buffer is no device buffer */
    if (ed25519_verify_keyed(ok, ks, (const uint32_t *)idx, sigs, msgs, NULL, 32, 0) != 0) { fprintf(stderr, "n = 0\n"); return 1; }
    if (ed25519_verify_keyed_dev(ok, ks, (const uint32_t *)idx, sigs, msgs, NULL, 32, n, NULL) == 0) { fprintf(stderr, "a host buffer passed as a device buffer\n"); return 1; }

    eddsa_amd_keyset_destroy(ks);
    eddsa_amd_keyset_destroy(NULL);
    eddsa_amd_shutdown();
    printf("verify_keyed: ok (%zu items, %zu keys)\n", n, count);
    free(ok); free(keys); free(idx); free(sigs); free(msgs); free(want);
    return 0;
}
