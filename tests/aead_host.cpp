// aead_host.cpp — the AES-256-GCM primitives of the device channel cipher
// (grapevine_amd/csrc/gvs_aead.h: key expansion, block function, GF(2^128)
// multiply, the serial whole-message form), built for the CPU so that
// tests/test_aead.py can check them against the openssl-made fixture without
// a GPU.  With -DAEAD_HOST_MAIN it is a stand-alone program (the GCM
// specification's test cases 13 and 14, a round trip at every length up to 300
// bytes and a rejection at each), which is what a sanitizer build runs.  Test
// infrastructure only.
#include "../grapevine_amd/csrc/gvs_aead.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace gvs;

// te0 from the S-box, the S-box from the field inverse (FIPS-197 §5.1.1)
static const uint32_t* te0_table() {
  static uint32_t te0[256];
  static bool made = false;
  if (made) return te0;
  auto xt = [](uint8_t v) { return (uint8_t)((v << 1) ^ ((v >> 7) * 0x1b)); };
  auto mul = [&](uint8_t a, uint8_t b) {
    uint8_t r = 0;
    for (; b; b >>= 1, a = xt(a))
      if (b & 1) r ^= a;
    return r;
  };
  for (int v = 0; v < 256; ++v) {
    uint8_t inv = 0;
    for (int c = 1; c < 256 && v; ++c)
      if (mul((uint8_t)v, (uint8_t)c) == 1) inv = (uint8_t)c;
    uint8_t s = inv, r = inv;
    for (int k = 0; k < 4; ++k) {
      r = (uint8_t)((r << 1) | (r >> 7));
      s ^= r;
    }
    s ^= 0x63;
    const uint8_t s2 = xt(s), s3 = (uint8_t)(s2 ^ s);
    te0[v] = (uint32_t)s2 << 24 | (uint32_t)s << 16 | (uint32_t)s << 8 | s3;
  }
  made = true;
  return te0;
}

extern "C" {

// out (len + 16 B) = C | tag
void aead_host_seal(const uint8_t* key, const uint8_t* iv, const uint8_t* aad, uint32_t aad_len,
                    const uint8_t* pt, uint32_t len, uint8_t* out) {
  aead_serial(true, te0_table(), key, iv, aad, aad_len, pt, len, out);
}

// in = C | tag (len B); out (len - 16 B) = P; returns 1, or 0 with out zeroed
int aead_host_open(const uint8_t* key, const uint8_t* iv, const uint8_t* aad, uint32_t aad_len,
                   const uint8_t* in, uint32_t len, uint8_t* out) {
  return aead_serial(false, te0_table(), key, iv, aad, aad_len, in, len, out) ? 1 : 0;
}
}

#ifdef AEAD_HOST_MAIN
static int fail(const char* what, unsigned at) {
  std::printf("aead_host: %s (%u)\n", what, at);
  return 1;
}

int main() {
  const uint8_t zero[32] = {};
  const uint8_t t13[16] = {0x53, 0x0f, 0x8a, 0xfb, 0xc7, 0x45, 0x36, 0xb9, 0xa9, 0x63, 0xb4, 0xf1, 0xc4, 0xcb, 0x73, 0x8b};
  const uint8_t t14[32] = {0xce, 0xa7, 0x40, 0x3d, 0x4d, 0x60, 0x6b, 0x6e, 0x07, 0x4e, 0xc5, 0xd3, 0xba, 0xf3, 0x9d, 0x18,
                           0xd0, 0xd1, 0xc8, 0xa7, 0x99, 0x99, 0x6b, 0xf0, 0x26, 0x5b, 0x98, 0xb5, 0xd4, 0x8a, 0xb9, 0x19};
  uint8_t out[48];
  aead_host_seal(zero, zero, nullptr, 0, nullptr, 0, out);
  if (std::memcmp(out, t13, 16)) return fail("test case 13", 0);
  aead_host_seal(zero, zero, nullptr, 0, zero, 16, out);
  if (std::memcmp(out, t14, 32)) return fail("test case 14", 0);
  uint32_t x = 1;
  auto rnd = [&] { return (uint8_t)((x = x * 1664525u + 1013904223u) >> 24); };
  for (uint32_t len = 0; len <= 300; ++len) {
    std::vector<uint8_t> key(32), iv(12), aad(len % 21), pt(len), ct(len + 16), back(len);
    for (auto* v : {&key, &iv, &aad, &pt})
      for (auto& b : *v) b = rnd();
    aead_host_seal(key.data(), iv.data(), aad.data(), (uint32_t)aad.size(), pt.data(), len, ct.data());
    if (!aead_host_open(key.data(), iv.data(), aad.data(), (uint32_t)aad.size(), ct.data(), len + 16, back.data()) ||
        back != pt)
      return fail("round trip", len);
    ct[len / 2] ^= 0x10;
    if (aead_host_open(key.data(), iv.data(), aad.data(), (uint32_t)aad.size(), ct.data(), len + 16, back.data()) ||
        back != std::vector<uint8_t>(len))
      return fail("rejection", len);
  }
  std::printf("aead_host ok\n");
  return 0;
}
#endif
