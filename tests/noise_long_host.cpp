// noise_long_host.cpp — the long Noise IX responder (grapevine_amd/csrc/
// gvs_noise_long.h) built for the CPU: noise_host.cpp's chain up to phase B,
// then k_noise_ix_tail's nt_item over rows laid out as the engine lays them
// out.  tests/test_noise_long.py checks it against grapevine_amd/noise.py.
// With -DNLHOST_MAIN it is a program of its own that runs the same lengths and
// the rejections (for a sanitizer build).  Test infrastructure only.
#include "noise_host.cpp"
#include "../grapevine_amd/csrc/gvs_noise_long.h"

extern "C" {

// One handshake.  msg2 holds msg2_stride bytes (a multiple of 16, >= 96 + p2)
// and is written whole; k1, k2 32 each; hh 64.  Returns the handshake's ok, or
// -1 if phase A's or B's lane states disagree.
int nx_long_host_respond(const uint8_t* s, const uint8_t* e, const uint8_t* pro, uint32_t pro_len,
                         const uint8_t* msg1, uint32_t msg1_len, const uint8_t* payload, uint32_t p2,
                         uint8_t* msg2, uint32_t msg2_stride, uint8_t* k1, uint8_t* k2, uint8_t* hh) {
  // uint4 rows: what the tail reads and writes in 16-byte words is 16-byte aligned
  std::vector<uint4> xout(10), st(8), ct1(3), ct2(nt_row(p2) / 16), slot2(msg2_stride / 16);
  std::vector<uint8_t> slot(128), cell(64), key(32), aad(64), text1(32), sealed(p2 + 16);
  if (msg1_len) std::memcpy(slot.data(), msg1, msg1_len < 128 ? msg1_len : 128);
  if (pro_len) std::memcpy(cell.data(), pro, pro_len);
  uint8_t* xo = (uint8_t*)xout.data();
  uint32_t xok[5], len1 = msg1_len, len2 = 0, ok = 0;
  const uint8_t* sc[5] = {e, e, e, s, s};
  const uint8_t* pt[5] = {nullptr, slot.data(), slot.data() + 32, slot.data(), nullptr};
  for (int k = 0; k < 5; ++k) {  // e_pub, ee, se, es, s_pub
    Fe r[4];
    x25519_quad_host(sc[k], pt[k], r);
    uint32_t any = 0;
    for (int i = 0; i < 32; ++i) any |= xo[32 * k + i] = (uint8_t)(r[0].v[i / 4] >> (8 * (i % 4)));
    xok[k] = any != 0;
  }
  NxArgs a{};
  a.n = 1, a.p2 = p2, a.steps_c = nt_steps(p2);
  a.msg1 = slot.data(), a.msg1_stride = 128, a.msg1_lens = &len1;
  a.pro = cell.data(), a.pro_len = pro_len;
  a.xout = xo, a.xok = xok;
  a.st = (uint8_t*)st.data(), a.key = key.data(), a.aad = aad.data(), a.text1 = text1.data();
  a.ct1 = (uint8_t*)ct1.data(), a.ct2 = (uint8_t*)ct2.data(), a.ct2_stride = nt_row(p2);
  a.msg2 = (uint8_t*)slot2.data(), a.msg2_stride = msg2_stride, a.msg2_lens = &len2;
  a.recv = k1, a.send = k2, a.hashes = hh, a.ok = &ok;
  const uint8_t iv[12] = {};
  bool agree = nx_item_host<kNxA>(a, 0);
  gvs::aead_serial(true, te0_table(), key.data(), iv, aad.data(), 64, text1.data(), 32, (uint8_t*)ct1.data());
  agree &= nx_item_host<kNxB>(a, 0);
  gvs::aead_serial(true, te0_table(), key.data(), iv, aad.data(), 64, payload, p2, sealed.data());
  std::memcpy(ct2.data(), sealed.data(), p2 + 16);  // the rest of the row stays zero, as k_aead_long leaves it
  for (uint32_t i = 0; i < a.n; ++i) nt_item(a, i);
  std::memcpy(msg2, slot2.data(), msg2_stride);
  if (!agree || len2 != (ok ? kNxMsg2Fixed + p2 : 0u)) return -1;
  return (int)ok;
}
}

#ifdef NLHOST_MAIN
static int nfail(const char* what, unsigned at) {
  std::printf("noise_long_host: %s (%u)\n", what, at);
  return 1;
}

int main() {  // tests/test_noise_long.py's lengths
  uint32_t x = 7;
  auto rnd = [&] { return (uint8_t)((x = x * 1664525u + 1013904223u) >> 24); };
  const uint32_t p2s[8] = {0, 31, 2048, 2049, 2079, 2080, 5000, kNxPayload2LongMax};
  uint8_t s[32], e[32], pro[64], m1[160], k1[32], k2[32], hh[64];
  std::vector<uint8_t> pay(kNxPayload2LongMax), msg2(65536), want(65536);
  int runs = 0;
  for (uint32_t l : {0u, 48u})
    for (uint32_t p2 : p2s) {
      for (auto& b : s) b = rnd();
      for (auto& b : e) b = rnd();
      for (auto& b : m1) b = rnd();
      for (auto& b : pro) b = rnd();
      for (auto& b : pay) b = rnd();
      const uint32_t stride = (96 + p2 + 15) / 16 * 16 + (p2 < 65000 ? 32 : 0);
      if (nx_long_host_respond(s, e, pro, l, m1, 64 + l, pay.data(), p2, msg2.data(), stride, k1, k2, hh) != 1)
        return nfail("handshake", p2);
      for (uint32_t i = 96 + p2; i < stride; ++i)
        if (msg2[i]) return nfail("the slot is not zero past the message", p2);
      uint8_t q1[32], q2[32], qh[64];  // the short form's bytes
      if (p2 <= 2048 && (nx_host_respond(s, e, pro, l, m1, 64 + l, pay.data(), p2, want.data(), q1, q2, qh) != 1 ||
                         std::memcmp(want.data(), msg2.data(), 96 + p2) || std::memcmp(q1, k1, 32) ||
                         std::memcmp(q2, k2, 32) || std::memcmp(qh, hh, 64)))
        return nfail("differs from the short form", p2);
      ++runs;
      for (int what = 0; what < 4; ++what) {  // both length limits, a small-order key in each position
        uint8_t bad[160];
        std::memcpy(bad, m1, sizeof bad);
        if (what >= 2) std::memset(bad + 32 * (what - 2), 0, 32);
        const uint32_t len = what == 0 ? 63 : what == 1 ? 129 : 64 + l;
        if (nx_long_host_respond(s, e, pro, l, bad, len, pay.data(), p2, msg2.data(), stride, k1, k2, hh) != 0)
          return nfail("rejection", what);
        uint32_t any = 0;
        for (uint32_t i = 0; i < stride; ++i) any |= msg2[i];
        for (int i = 0; i < 32; ++i) any |= k1[i] | k2[i] | hh[i] | hh[32 + i];
        if (any) return nfail("a rejected handshake's outputs are not zero", what);
      }
    }
  std::printf("noise_long_host ok: %d handshakes, 4 rejections each\n", runs);
  return 0;
}
#endif
