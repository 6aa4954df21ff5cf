/* TEST PROGRAM: the host side linked WITHOUT the HIP translation unit (tests/fake_hip: a fake runtime and CPU launchers that know
 * no [m]P + [a]B pass).  The launcher of edk_muladd.h is a weak reference there: both forms of ed25519_point_muladd_batch
 * (include/eddsa_amd.h) answer -hipErrorNotSupported in each of the four ways to call, the argument checks in front of that answer as
 * everywhere, the output untouched, and the fake runtime holds no allocation afterwards.  Built and run by
 * tests/test_point_muladd_on_host.py. */
#include <stdio.h>
#include <stdint.h>
#include <string.h>

#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include "eddsa_amd.h"
#include "fake_hip.h"

int main(void)
{
    uint8_t points[4 * 32], mul[4 * 32], add[4 * 32], out[4 * 32], *d[4] = { NULL, NULL, NULL, NULL };
    int failures = 0, rc;
    memset(points, 7, sizeof(points));
    memset(mul, 3, sizeof(mul));
    memset(add, 5, sizeof(add));
    memset(out, 0xee, sizeof(out));

    for (int k = 0; k < 4; k++) {                                /* through the staging pipeline of (fake) device 0 */
        rc = ed25519_point_muladd_batch(out, points, k & 1 ? mul : NULL, k & 2 ? add : NULL, 4);
        if (rc != -(int)hipErrorNotSupported) { printf("host form %d: rc %d\n", k, rc); failures++; }
    }
    if (ed25519_point_muladd_batch(NULL, points, mul, add, 4) != -(int)hipErrorInvalidValue) { printf("host form, NULL out\n"); failures++; }
    if (ed25519_point_muladd_batch(out, NULL, mul, add, 4) != -(int)hipErrorInvalidValue) { printf("host form, NULL points\n"); failures++; }
    if (ed25519_point_muladd_batch(NULL, NULL, NULL, NULL, 0) != 0) { printf("host form, empty\n"); failures++; }

    for (int k = 0; k < 4; k++)
        if (hipMalloc((void **)&d[k], sizeof(points)) != hipSuccess) { printf("hipMalloc failed\n"); return 2; }
    for (int k = 0; k < 4; k++) {
        rc = ed25519_point_muladd_batch_dev(d[0], d[1], k & 1 ? d[2] : NULL, k & 2 ? d[3] : NULL, 4, NULL);
        if (rc != -(int)hipErrorNotSupported) { printf("device form %d: rc %d\n", k, rc); failures++; }
    }
    if (ed25519_point_muladd_batch_dev(NULL, d[1], d[2], d[3], 4, NULL) != -(int)hipErrorInvalidValue) { printf("device form, NULL out\n"); failures++; }
    if (ed25519_point_muladd_batch_dev(d[0], NULL, d[2], d[3], 4, NULL) != -(int)hipErrorInvalidValue) { printf("device form, NULL points\n"); failures++; }
    if (ed25519_point_muladd_batch_dev(NULL, NULL, NULL, NULL, 0, NULL) != 0) { printf("device form, empty\n"); failures++; }
    for (int k = 0; k < 4; k++) (void)hipFree(d[k]);

    for (size_t k = 0; k < sizeof(out); k++) if (out[k] != 0xee) { printf("out was written\n"); failures++; break; }
    eddsa_amd_shutdown();
    {
        const long live = fake_hip_live_allocations();
        if (live != 0) { printf("%ld allocations of the fake runtime are still live\n", live); failures++; }
    }
    printf(failures ? "FAILED\n" : "muladd_without_kernels ok\n");
    return failures != 0;
}
