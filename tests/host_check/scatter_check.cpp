// scatter_check.cpp - TEST BINARY: the span test and the lane of k_scatter_challenge (libeddsa_amd/csrc/scatter_lanes.h:
// scatter_item_inside, scatter_item_len, scatter_challenge_lane), the front of ed25519_verify_scattered (include/eddsa_amd.h),
// compiled for the host CPU with -DED_HOST_CHECK (every bound asserted).  Built by tests/test_scattered_on_host.py twice: as a
// library for ctypes, and with -DSCATTER_CHECK_MAIN -fsanitize=address,undefined as a program of its own that reads its cases from
// a file and holds the data buffer in an allocation of exactly data_len rounded up to 4 bytes.  Not part of the product.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "scatter_lanes.h"

namespace ed {
static std::atomic<long> g_violations{0};
void bound_violation(const char* file, int line, const char* what) {
  if (g_violations.fetch_add(1) == 0) fprintf(stderr, "bound violated: %s:%d: %s\n", file, line, what);
}
}  // namespace ed

using namespace ed;

extern "C" {

long sc_violations(void) { return g_violations.load(); }

int sc_inside(uint32_t sig_off, uint32_t pub_off, uint32_t msg_off, uint32_t msg_len, uint64_t data_len) {
  return (int)scatter_item_inside(sig_off, pub_off, msg_off, msg_len, data_len);
}
uint32_t sc_len(uint32_t sig_off, uint32_t pub_off, uint32_t msg_off, uint32_t msg_len, uint64_t data_len) {
  return scatter_item_len(sig_off, pub_off, msg_off, msg_len, data_len);
}

// both over n items at once: inside[i] and len[i]
void sc_spans(uint8_t* inside, uint32_t* len, const uint32_t* sig_off, const uint32_t* pub_off, const uint32_t* msg_off,
              const uint32_t* msg_len, size_t n, uint64_t data_len) {
  for (size_t i = 0; i < n; i++) {
    inside[i] = (uint8_t)scatter_item_inside(sig_off[i], pub_off[i], msg_off[i], msg_len[i], data_len);
    len[i] = scatter_item_len(sig_off[i], pub_off[i], msg_off[i], msg_len[i], data_len);
  }
}

// one item through the lane: sig (64 bytes), key (32), dig (64) as the kernel's slots receive them, dirtied first - the lane must
// write all of them.  Returns what the lane returns
int sc_lane(uint8_t* sig, uint8_t* key, uint8_t* dig, const uint8_t* data, uint64_t data_len, uint32_t sig_off, uint32_t pub_off,
            uint32_t msg_off, uint32_t msg_len) {
  alignas(16) uint32_t s[16], k[8], d[16];
  memset(s, 0xa5, sizeof(s)); memset(k, 0xa5, sizeof(k)); memset(d, 0xa5, sizeof(d));
  const bool in = scatter_challenge_lane(s, k, d, data, data_len, sig_off, pub_off, msg_off, msg_len);
  memcpy(sig, s, 64); memcpy(key, k, 32); memcpy(dig, d, 64);      // little-endian host
  return (int)in;
}

}  // extern "C"

#ifdef SCATTER_CHECK_MAIN
// scatter_check cases.bin - the file: data_len (u32), data_len bytes, the number of cases (u32), then per case sig_off, pub_off,
// msg_off, msg_len (u32 each) and the 64 bytes SHA-512(R || A || M) the writer expects (ignored for an item outside the buffer).
// The buffer is copied into an allocation of data_len rounded up to 4 bytes and handed to the lane THERE: the words the header
// documents are the allocation, and AddressSanitizer reports any byte read beyond them.
static uint32_t u32(FILE* f) {
  uint32_t v;
  if (fread(&v, 4, 1, f) != 1) { fprintf(stderr, "short file\n"); exit(2); }
  return v;
}
int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  const uint32_t data_len = u32(f);
  uint8_t* data = static_cast<uint8_t*>(malloc(((size_t)data_len + 3) & ~(size_t)3));
  if (!data || (data_len && fread(data, 1, data_len, f) != data_len)) { fprintf(stderr, "short file\n"); return 2; }
  const uint32_t cases = u32(f);
  long bad = 0, inside = 0;
  for (uint32_t c = 0; c < cases; c++) {
    const uint32_t so = u32(f), po = u32(f), mo = u32(f), ml = u32(f);
    uint8_t want[64], sig[64], key[32], dig[64], zero[64] = {0}, nokey[32] = {2};
    if (fread(want, 1, 64, f) != 64) { fprintf(stderr, "short file\n"); return 2; }
    const int in = sc_lane(sig, key, dig, data, data_len, so, po, mo, ml);
    const bool expect_in = (uint64_t)so + 64 <= data_len && (uint64_t)po + 32 <= data_len && (uint64_t)mo + ml <= data_len;
    bool good = in == (int)expect_in;
    if (expect_in) good = good && !memcmp(sig, data + so, 64) && !memcmp(key, data + po, 32) && !memcmp(dig, want, 64);
    else good = good && !memcmp(sig, zero, 64) && !memcmp(dig, zero, 64) && !memcmp(key, nokey, 32);
    if (!good && bad++ == 0) fprintf(stderr, "case %u (%u, %u, %u, %u) differs\n", c, so, po, mo, ml);
    inside += in;
  }
  fclose(f);
  free(data);
  if (bad || sc_violations()) { printf("scatter_check: %ld cases differ, %ld bounds violated\n", bad, sc_violations()); return 1; }
  printf("scatter_check: ok (%u cases, %ld inside)\n", cases, inside);
  return 0;
}
#endif
