/* verify_scattered.c - a plain C caller of ed25519_verify_scattered (include/eddsa_amd.h) against the SHIPPED library:
 *   verify_scattered data.bin sig_off.bin pub_off.bin msg_off.bin msg_len.bin want.bin
 * data.bin is the buffer, the four index files hold n uint32 each, want.bin the n verdict bytes the oracle gives for the gathered
 * spans; tests/test_gpu_scattered.py writes them.  Exit status 0 and "verify_scattered: ok" when the call returns exactly those
 * bytes and leaves their neighbours alone, and refuses a span that leaves the buffer, a NULL array and a buffer of 2^32 bytes
 * without writing a verdict. */
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

static int untouched(const uint8_t *buf, size_t n)
{
    for (size_t i = 0; i < n + 2; i++) if (buf[i] != 0xee) return 0;
    return 1;
}

int main(int argc, char **argv)
{
    if (argc != 7) { fprintf(stderr, "usage: %s data sig_off pub_off msg_off msg_len want\n", argv[0]); return 2; }
    size_t len[6];
    uint8_t *f[6];
    for (int k = 0; k < 6; k++) f[k] = slurp(argv[1 + k], &len[k]);
    const size_t n = len[5], data_len = len[0];
    for (int k = 1; k < 5; k++) if (len[k] != 4 * n || n == 0) { fprintf(stderr, "the files disagree on the number of items\n"); return 2; }
    const uint8_t *data = f[0], *want = f[5];
    uint32_t *idx[4];
    for (int k = 0; k < 4; k++) idx[k] = (uint32_t *)f[1 + k];
    uint8_t *buf = malloc(n + 2), *ok = buf + 1;     /* an odd address, a guard byte on either side */
    int rc;
    if (!buf) return 2;

    memset(buf, 0xee, n + 2);
    if ((rc = ed25519_verify_scattered(ok, data, data_len, idx[0], idx[1], idx[2], idx[3], n)) != 0) {
        fprintf(stderr, "ed25519_verify_scattered: %s\n", eddsa_amd_strerror(rc));
        return 1;
    }
    for (size_t i = 0; i < n; i++) if (ok[i] != want[i]) { fprintf(stderr, "item %zu: %d, expected %d\n", i, ok[i], want[i]); return 1; }
    if (buf[0] != 0xee || buf[n + 1] != 0xee) { fprintf(stderr, "a neighbour of ok was written\n"); return 1; }

    /* refusals: nothing is written */
    memset(buf, 0xee, n + 2);
    const uint32_t keep = idx[2][n / 2];
    idx[2][n / 2] = (uint32_t)data_len;              /* a message (of any length > 0) that starts where the buffer ends */
    const uint32_t keep_len = idx[3][n / 2];
    idx[3][n / 2] = 1;
    if (ed25519_verify_scattered(ok, data, data_len, idx[0], idx[1], idx[2], idx[3], n) >= 0 || !untouched(buf, n)) {
        fprintf(stderr, "a span outside the buffer was not refused\n"); return 1;
    }
    idx[2][n / 2] = keep; idx[3][n / 2] = keep_len;
    if (ed25519_verify_scattered(ok, data, data_len, idx[0], NULL, idx[2], idx[3], n) >= 0 ||
        ed25519_verify_scattered(NULL, data, data_len, idx[0], idx[1], idx[2], idx[3], n) >= 0 ||
        ed25519_verify_scattered(ok, data, (size_t)1 << 32, idx[0], idx[1], idx[2], idx[3], n) >= 0 ||
        ed25519_verify_scattered(NULL, NULL, 0, NULL, NULL, NULL, NULL, 0) != 0 || !untouched(buf, n)) {
        fprintf(stderr, "the argument checks\n"); return 1;
    }

    eddsa_amd_shutdown();
    printf("verify_scattered: ok (%zu items)\n", n);
    for (int k = 0; k < 6; k++) free(f[k]);
    free(buf);
    return 0;
}
