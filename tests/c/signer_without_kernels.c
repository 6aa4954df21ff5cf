/* TEST PROGRAM: the host side linked WITHOUT the HIP translation unit (tests/fake_hip: a fake runtime and CPU launchers that know
 * no signer sets).  The launchers of edk_signer.h are weak references there: creating a signer set answers
 * -hipErrorNotSupported and leaves *out NULL; the argument checks in front of it answer as everywhere.  Built and run by
 * tests/test_sign_keyed_on_host.py. */
#include <stdio.h>
#include <stdint.h>
#include <string.h>

#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include "eddsa_amd.h"

int main(void)
{
    uint8_t keys[4 * 64];
    int failures = 0;
    memset(keys, 7, sizeof(keys));
    eddsa_amd_signer *s = (eddsa_amd_signer *)keys;
    int rc = eddsa_amd_signer_create(&s, keys, 4);
    if (rc != -(int)hipErrorNotSupported || s != NULL) { printf("create: rc %d, out %p\n", rc, (void *)s); failures++; }
    s = (eddsa_amd_signer *)keys;
    rc = eddsa_amd_signer_create_expanded(&s, keys, 4);
    if (rc != -(int)hipErrorNotSupported || s != NULL) { printf("create_expanded: rc %d, out %p\n", rc, (void *)s); failures++; }
    s = (eddsa_amd_signer *)keys;
    rc = eddsa_amd_signer_create(&s, keys, 0);
    if (rc != -(int)hipErrorInvalidValue || s != NULL) { printf("create, count 0: rc %d\n", rc); failures++; }
    eddsa_amd_signer_destroy(NULL);
    eddsa_amd_shutdown();
    printf(failures ? "FAILED\n" : "signer_without_kernels ok\n");
    return failures != 0;
}
