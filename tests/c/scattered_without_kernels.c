/* TEST PROGRAM: the host side linked WITHOUT the HIP translation unit (tests/fake_hip: a fake runtime and CPU launchers that know
 * no scattered pass).  The launcher of edk_scatter.h is a weak reference there: both forms of ed25519_verify_scattered
 * (include/eddsa_amd.h) answer -hipErrorNotSupported, the argument checks in front of that answer as everywhere, the output
 * untouched, and the fake runtime holds no allocation afterwards.  Built and run by tests/test_scattered_on_host.py. */
#include <stdio.h>
#include <stdint.h>
#include <string.h>

#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include "eddsa_amd.h"
#include "fake_hip.h"

int main(void)
{
    uint8_t data[4 * 128], ok[4], *d_ok = NULL, *d_data = NULL;
    uint32_t so[4], po[4], mo[4], ml[4], *d_idx = NULL;
    int failures = 0, rc;
    memset(data, 7, sizeof(data));
    memset(ok, 0xee, sizeof(ok));
    for (uint32_t i = 0; i < 4; i++) { so[i] = 128 * i; po[i] = 128 * i + 64; mo[i] = 128 * i + 96; ml[i] = 32; }

    rc = ed25519_verify_scattered(ok, data, sizeof(data), so, po, mo, ml, 4);
    if (rc != -(int)hipErrorNotSupported) { printf("host form: rc %d\n", rc); failures++; }
    if (ed25519_verify_scattered(NULL, data, sizeof(data), so, po, mo, ml, 4) != -(int)hipErrorInvalidValue) { printf("host form, NULL ok\n"); failures++; }
    if (ed25519_verify_scattered(ok, data, sizeof(data), so, NULL, mo, ml, 4) != -(int)hipErrorInvalidValue) { printf("host form, NULL pub_off\n"); failures++; }
    if (ed25519_verify_scattered(ok, data, (size_t)1 << 32, so, po, mo, ml, 4) != -(int)hipErrorInvalidValue) { printf("host form, 2^32\n"); failures++; }
    if (ed25519_verify_scattered(NULL, NULL, 0, NULL, NULL, NULL, NULL, 0) != 0) { printf("host form, empty\n"); failures++; }

    if (hipMalloc((void **)&d_ok, 4) != hipSuccess || hipMalloc((void **)&d_data, sizeof(data)) != hipSuccess ||
        hipMalloc((void **)&d_idx, 16 * sizeof(uint32_t)) != hipSuccess) { printf("hipMalloc failed\n"); return 2; }
    rc = ed25519_verify_scattered_dev(d_ok, d_data, sizeof(data), d_idx, d_idx + 4, d_idx + 8, d_idx + 12, 4, NULL);
    if (rc != -(int)hipErrorNotSupported) { printf("device form: rc %d\n", rc); failures++; }
    if (ed25519_verify_scattered_dev(d_ok, NULL, sizeof(data), d_idx, d_idx + 4, d_idx + 8, d_idx + 12, 4, NULL) != -(int)hipErrorInvalidValue) {
        printf("device form, NULL data\n"); failures++;
    }
    if (ed25519_verify_scattered_dev(d_ok, d_data, (size_t)1 << 32, d_idx, d_idx + 4, d_idx + 8, d_idx + 12, 4, NULL) != -(int)hipErrorInvalidValue) {
        printf("device form, 2^32\n"); failures++;
    }
    if (ed25519_verify_scattered_dev(NULL, NULL, 0, NULL, NULL, NULL, NULL, 0, NULL) != 0) { printf("device form, empty\n"); failures++; }
    (void)hipFree(d_ok); (void)hipFree(d_data); (void)hipFree(d_idx);

    for (size_t k = 0; k < sizeof(ok); k++) if (ok[k] != 0xee) { printf("ok was written\n"); failures++; break; }
    eddsa_amd_shutdown();
    {
        const long live = fake_hip_live_allocations();
        if (live != 0) { printf("%ld allocations of the fake runtime are still live\n", live); failures++; }
    }
    printf(failures ? "FAILED\n" : "scattered_without_kernels ok\n");
    return failures != 0;
}
