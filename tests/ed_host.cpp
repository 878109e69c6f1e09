// ed_host.cpp — the SHA-512, the strict Edwards decoding and the whole
// per-thread check of the device Ed25519 verification
// (grapevine_amd/csrc/gvs_ed25519.h, host-callable), built for the CPU so
// that tests/test_ed_host.py can check them against hashlib and the oracle
// (oracle/sr25519.py) without a GPU.  Test infrastructure only.
#include "../grapevine_amd/csrc/gvs_ed25519.h"

using namespace gvs::sr;

extern "C" {

// out (64 B) = SHA-512(in[0:len]), the input cut into the routine's three
// pieces at bytes 32 and 64 as a signature's R, A and M are
void ed_host_sha512(const uint8_t* in, uint32_t len, uint8_t* out) {
  const uint32_t n0 = len < 32 ? len : 32, n1 = len - n0 < 32 ? len - n0 : 32;
  uint32_t w[16];
  sha512_3(Sha512In{in, n0, in + n0, n1, in + n0 + n1, len - n0 - n1}, w, 1);
  for (int i = 0; i < 64; ++i) out[i] = (uint8_t)(w[i / 4] >> (8 * (i % 4)));
}

// out_xy (64 B) = canonical x, y of decode(in); returns the verdict (1 ok)
int ed_host_decode(const uint8_t* in, uint8_t* out_xy) {
  Fe b;
  for (int i = 0; i < 8; ++i) b.v[i] = ld_le32(in + 4 * i);
  uint32_t ok = 0;
  const Pt p = ed_decode(b, &ok);
  const Fe x = fe_canon(p.X), y = fe_canon(p.Y);
  for (int i = 0; i < 32; ++i) {
    out_xy[i] = (uint8_t)(x.v[i / 4] >> (8 * (i % 4)));
    out_xy[32 + i] = (uint8_t)(y.v[i / 4] >> (8 * (i % 4)));
  }
  return ok ? 1 : 0;
}

// the whole check of one signature; 1 valid
int ed_host_verify(const uint8_t* pk, const uint8_t* msg, uint32_t len, const uint8_t* sig) {
  return ed_verify_host(pk, msg, len, sig) ? 1 : 0;
}
}
