/* TEST PROGRAM: the host side linked WITHOUT the HIP translation unit (tests/fake_hip: a fake runtime and CPU launchers that know
 * no point classification).  The launcher of edk_classify.h is a weak reference there: the three calls of include/eddsa_amd.h's
 * point classification answer -hipErrorNotSupported, the argument checks in front of that answer as everywhere, and the fake
 * runtime holds no allocation afterwards.  Built and run by tests/test_classify_on_host.py. */
#include <stdio.h>
#include <stdint.h>
#include <string.h>

#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include "eddsa_amd.h"
#include "fake_hip.h"

int main(void)
{
    uint8_t points[4 * 32], cls[4], *d_points = NULL, *d_cls = NULL;
    int failures = 0, rc;
    memset(points, 7, sizeof(points));
    memset(cls, 0xee, sizeof(cls));

    rc = ed25519_point_classify_batch(cls, points, 4);                       /* through the staging pipeline of (fake) device 0 */
    if (rc != -(int)hipErrorNotSupported) { printf("host form: rc %d\n", rc); failures++; }
    if (ed25519_point_classify_batch(NULL, points, 4) != -(int)hipErrorInvalidValue) { printf("host form, NULL cls\n"); failures++; }
    if (ed25519_point_classify_batch(cls, NULL, 4) != -(int)hipErrorInvalidValue) { printf("host form, NULL points\n"); failures++; }
    if (ed25519_point_classify_batch(NULL, NULL, 0) != 0) { printf("host form, empty\n"); failures++; }

    if (hipMalloc((void **)&d_points, sizeof(points)) != hipSuccess || hipMalloc((void **)&d_cls, sizeof(cls)) != hipSuccess) {
        printf("hipMalloc failed\n");
        return 2;
    }
    rc = ed25519_point_classify_batch_dev(d_cls, d_points, 4, NULL);
    if (rc != -(int)hipErrorNotSupported) { printf("device form: rc %d\n", rc); failures++; }
    if (ed25519_point_classify_batch_dev(NULL, d_points, 4, NULL) != -(int)hipErrorInvalidValue) { printf("device form, NULL cls\n"); failures++; }
    if (ed25519_point_classify_batch_dev(d_cls, NULL, 4, NULL) != -(int)hipErrorInvalidValue) { printf("device form, NULL points\n"); failures++; }
    if (ed25519_point_classify_batch_dev(NULL, NULL, 0, NULL) != 0) { printf("device form, empty\n"); failures++; }
    (void)hipFree(d_points);
    (void)hipFree(d_cls);

    /* no key set can exist here (creating one is -hipErrorNotSupported as well): the handle is never looked into */
    {
        eddsa_amd_keyset *ks = (eddsa_amd_keyset *)points;
        if (eddsa_amd_keyset_create(&ks, points, 4) != -(int)hipErrorNotSupported || ks != NULL) { printf("keyset_create\n"); failures++; }
        rc = eddsa_amd_keyset_classify((const eddsa_amd_keyset *)points, cls);
        if (rc != -(int)hipErrorNotSupported) { printf("keyset form: rc %d\n", rc); failures++; }
        if (eddsa_amd_keyset_classify(NULL, cls) != -(int)hipErrorInvalidValue) { printf("keyset form, NULL ks\n"); failures++; }
        if (eddsa_amd_keyset_classify((const eddsa_amd_keyset *)points, NULL) != -(int)hipErrorInvalidValue) { printf("keyset form, NULL cls\n"); failures++; }
    }
    eddsa_amd_shutdown();
    {
        const long live = fake_hip_live_allocations();
        if (live != 0) { printf("%ld allocations of the fake runtime are still live\n", live); failures++; }
    }
    printf(failures ? "FAILED\n" : "classify_without_kernels ok\n");
    return failures != 0;
}
