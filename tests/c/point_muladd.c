/* point_muladd.c - a plain C caller of ed25519_point_muladd_batch (include/eddsa_amd.h) against the SHIPPED library:
 *   point_muladd points.bin mul.bin add.bin want.bin want_mul.bin want_add.bin want_points.bin
 * The files hold n packed items of 32 bytes; tests/test_gpu_point_muladd.py writes them, with what tests/point_muladd_model.py expects
 * of the four ways to call: both scalar arrays, mul alone, add alone, neither.  Exit status 0 and "point_muladd: ok" when the four
 * calls - the last one in place - return exactly those bytes and leave their neighbours alone. */
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
        if (memcmp(got + 32 * i, want + 32 * i, 32)) { fprintf(stderr, "%s: item %zu differs\n", what, i); return 0; }
    return 1;
}

int main(int argc, char **argv)
{
    if (argc != 8) { fprintf(stderr, "usage: %s points mul add want want_mul want_add want_points\n", argv[0]); return 2; }
    size_t len[7];
    uint8_t *f[7];
    for (int k = 0; k < 7; k++) f[k] = slurp(argv[1 + k], &len[k]);
    const size_t n = len[0] / 32;
    for (int k = 0; k < 7; k++) if (len[k] != 32 * n || n == 0) { fprintf(stderr, "the files disagree on the number of items\n"); return 2; }
    const uint8_t *points = f[0], *mul = f[1], *add = f[2];
    uint8_t *buf = malloc(32 * n + 2), *out = buf + 1;   /* an odd address, a guard byte on either side */
    int rc;
    if (!buf) return 2;

    const struct { const char *what; const uint8_t *mul, *add, *want; } calls[3] = {
        { "mul and add", mul, add, f[3] }, { "mul alone", mul, NULL, f[4] }, { "add alone", NULL, add, f[5] } };
    for (int k = 0; k < 3; k++) {
        memset(buf, 0xee, 32 * n + 2);
        if ((rc = ed25519_point_muladd_batch(out, points, calls[k].mul, calls[k].add, n)) != 0) {
            fprintf(stderr, "ed25519_point_muladd_batch (%s): %s\n", calls[k].what, eddsa_amd_strerror(rc));
            return 1;
        }
        if (!same(calls[k].what, out, calls[k].want, n)) return 1;
        if (buf[0] != 0xee || buf[32 * n + 1] != 0xee) { fprintf(stderr, "%s: a neighbour of out was written\n", calls[k].what); return 1; }
    }
    /* neither array, in place: the canonical re-encoding of every point */
    memcpy(out, points, 32 * n);
    if ((rc = ed25519_point_muladd_batch(out, out, NULL, NULL, n)) != 0) { fprintf(stderr, "in place: %s\n", eddsa_amd_strerror(rc)); return 1; }
    if (!same("in place", out, f[6], n)) return 1;
    if (buf[0] != 0xee || buf[32 * n + 1] != 0xee) { fprintf(stderr, "in place: a neighbour of out was written\n"); return 1; }
    if (EDDSA_AMD_NO_POINT_BYTE0 != 0x02) return 1;

    if (ed25519_point_muladd_batch(NULL, points, mul, add, n) >= 0 || ed25519_point_muladd_batch(out, NULL, mul, add, n) >= 0 ||
        ed25519_point_muladd_batch(NULL, NULL, NULL, NULL, 0) != 0) { fprintf(stderr, "the argument checks\n"); return 1; }

    eddsa_amd_shutdown();
    printf("point_muladd: ok (%zu items)\n", n);
    for (int k = 0; k < 7; k++) free(f[k]);
    free(buf);
    return 0;
}
