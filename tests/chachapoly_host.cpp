// chachapoly_host.cpp — the ChaCha20-Poly1305 primitives of the device channel
// cipher (grapevine_amd/csrc/gvs_chachapoly.h: the RFC 8439 block function,
// the Poly1305 multiply, carry and finish, the serial whole-message form),
// built for the CPU so that tests/test_chachapoly.py can check them against
// RFC 8439's vectors and the openssl-made fixture without a GPU.  With
// -DCHACHAPOLY_HOST_MAIN it is a stand-alone program (RFC 8439 §2.5.2, a
// round trip at every length up to 300 bytes and a rejection at each), which
// is what a sanitizer build runs.  Test infrastructure only.
#include "../grapevine_amd/csrc/gvs_chachapoly.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace gvs;

extern "C" {

// out (len + 16 B) = C | tag
void chachapoly_host_seal(const uint8_t* key, const uint8_t* nonce, const uint8_t* aad, uint32_t aad_len,
                          const uint8_t* pt, uint32_t len, uint8_t* out) {
  chachapoly_item(true, key, nonce, aad, aad_len, pt, len, out);
}

// in = C | tag (len B); out (len - 16 B) = P; returns 1, or 0 with out zeroed
int chachapoly_host_open(const uint8_t* key, const uint8_t* nonce, const uint8_t* aad, uint32_t aad_len,
                         const uint8_t* in, uint32_t len, uint8_t* out) {
  return chachapoly_item(false, key, nonce, aad, aad_len, in, len, out) ? 1 : 0;
}

// tag (16 B) = Poly1305 of msg under the 32-byte one-time key
void chachapoly_host_poly1305(const uint8_t* key, const uint8_t* msg, uint32_t len, uint8_t* tag) {
  poly1305(key, msg, len, tag);
}
}

#ifdef CHACHAPOLY_HOST_MAIN
static int fail(const char* what, unsigned at) {
  std::printf("chachapoly_host: %s (%u)\n", what, at);
  return 1;
}

int main() {
  // RFC 8439 §2.5.2
  const uint8_t pk[32] = {0x85, 0xd6, 0xbe, 0x78, 0x57, 0x55, 0x6d, 0x33, 0x7f, 0x44, 0x52, 0xfe, 0x42, 0xd5, 0x06, 0xa8,
                          0x01, 0x03, 0x80, 0x8a, 0xfb, 0x0d, 0xb2, 0xfd, 0x4a, 0xbf, 0xf6, 0xaf, 0x41, 0x49, 0xf5, 0x1b};
  const char* pm = "Cryptographic Forum Research Group";
  const uint8_t pt_want[16] = {0xa8, 0x06, 0x1d, 0xc1, 0x30, 0x51, 0x36, 0xc6, 0xc2, 0x2b, 0x8b, 0xaf, 0x0c, 0x01, 0x27, 0xa9};
  uint8_t tag[16];
  chachapoly_host_poly1305(pk, (const uint8_t*)pm, 34, tag);
  if (std::memcmp(tag, pt_want, 16)) return fail("RFC 8439 2.5.2", 0);
  uint32_t x = 1;
  auto rnd = [&] { return (uint8_t)((x = x * 1664525u + 1013904223u) >> 24); };
  for (uint32_t len = 0; len <= 300; ++len) {
    std::vector<uint8_t> k(32), n(12), a(len % 21), pt(len), ct(len + 16), back(len);
    for (auto* v : {&k, &n, &a, &pt})
      for (auto& b : *v) b = rnd();
    chachapoly_host_seal(k.data(), n.data(), a.data(), (uint32_t)a.size(), pt.data(), len, ct.data());
    if (!chachapoly_host_open(k.data(), n.data(), a.data(), (uint32_t)a.size(), ct.data(), len + 16, back.data()) ||
        back != pt)
      return fail("round trip", len);
    ct[len / 2] ^= 0x10;
    if (chachapoly_host_open(k.data(), n.data(), a.data(), (uint32_t)a.size(), ct.data(), len + 16, back.data()) ||
        back != std::vector<uint8_t>(len))
      return fail("rejection", len);
  }
  std::printf("chachapoly_host ok\n");
  return 0;
}
#endif
