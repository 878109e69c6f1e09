// noise_host.cpp — the device Noise IX responder (grapevine_amd/csrc/
// gvs_noise.h) built for the CPU: the three phases of k_noise_ix stepped over
// four lane states, chained with x25519_quad_host and aead_serial the way
// gvs_noise_ix_respond chains the kernels.  tests/test_noise.py checks it
// against grapevine_amd/noise.py without a GPU.  With -DNHOST_MAIN it is a
// program of its own that runs the padding-edge lengths and the rejections
// (for a sanitizer build).  Test infrastructure only.
#include "aead_host.cpp"  // te0_table
#include "../grapevine_amd/csrc/gvs_noise.h"

using namespace gvs::sr;

extern "C" {

// One handshake.  msg2 holds 96 + p2 bytes; k1, k2 32 each; hh 64.  Returns
// the handshake's ok (0 or 1), or -1 if lane states that hold the same value
// disagree in any phase.
int nx_host_respond(const uint8_t* s, const uint8_t* e, const uint8_t* pro, uint32_t pro_len,
                    const uint8_t* msg1, uint32_t msg1_len, const uint8_t* payload, uint32_t p2,
                    uint8_t* msg2, uint8_t* k1, uint8_t* k2, uint8_t* hh) {
  std::vector<uint8_t> slot(128), cell(64), xout(5 * 32), st(128), key(32), aad(64), text1(32), ct1(48),
      ct2(p2 + 16);
  if (msg1_len) std::memcpy(slot.data(), msg1, msg1_len < 128 ? msg1_len : 128);
  if (pro_len) std::memcpy(cell.data(), pro, pro_len);
  uint32_t xok[5], len1 = msg1_len, len2 = 0, ok = 0;
  const uint8_t* sc[5] = {e, e, e, s, s};
  const uint8_t* pt[5] = {nullptr, slot.data(), slot.data() + 32, slot.data(), nullptr};
  for (int k = 0; k < 5; ++k) {  // e_pub, ee, se, es, s_pub
    Fe r[4];
    x25519_quad_host(sc[k], pt[k], r);
    uint32_t any = 0;
    for (int i = 0; i < 32; ++i) any |= xout[32 * k + i] = (uint8_t)(r[0].v[i / 4] >> (8 * (i % 4)));
    xok[k] = any != 0;
  }
  NxArgs a{};
  a.n = 1, a.p2 = p2, a.steps_c = nx_steps_c(p2);
  a.msg1 = slot.data(), a.msg1_stride = 128, a.msg1_lens = &len1;
  a.pro = cell.data(), a.pro_len = pro_len;
  a.xout = xout.data(), a.xok = xok;
  a.st = st.data(), a.key = key.data(), a.aad = aad.data(), a.text1 = text1.data();
  a.ct1 = ct1.data(), a.ct2 = ct2.data(), a.ct2_stride = p2 + 16;
  a.msg2 = msg2, a.msg2_stride = kNxMsg2Fixed + p2, a.msg2_lens = &len2;
  a.recv = k1, a.send = k2, a.hashes = hh, a.ok = &ok;
  const uint8_t iv[12] = {};
  bool agree = nx_item_host<kNxA>(a, 0);
  gvs::aead_serial(true, te0_table(), key.data(), iv, aad.data(), 64, text1.data(), 32, ct1.data());
  agree &= nx_item_host<kNxB>(a, 0);
  gvs::aead_serial(true, te0_table(), key.data(), iv, aad.data(), 64, payload, p2, ct2.data());
  agree &= nx_item_host<kNxC>(a, 0);
  if (!agree || len2 != (ok ? kNxMsg2Fixed + p2 : 0u)) return -1;
  return (int)ok;
}
}

#ifdef NHOST_MAIN
static int nfail(const char* what, unsigned at) {
  std::printf("noise_host: %s (%u)\n", what, at);
  return 1;
}

int main() {
  uint32_t x = 7;
  auto rnd = [&] { return (uint8_t)((x = x * 1664525u + 1013904223u) >> 24); };
  const uint32_t edge[4] = {0, 47, 48, 64}, p2s[7] = {0, 1, 31, 32, 159, 160, 2048};
  uint8_t s[32], e[32], pro[64], m1[160], k1[32], k2[32], hh[64];
  std::vector<uint8_t> pay(2048), msg2(96 + 2048);
  int runs = 0;
  for (uint32_t pl : edge)
    for (uint32_t l1 : edge)
      for (uint32_t p2 : p2s) {
        if (!(p2 == 31 || (pl == l1 && (pl == 0 || pl == 48)))) continue;
        for (auto& b : s) b = rnd();
        for (auto& b : e) b = rnd();
        for (auto& b : pro) b = rnd();
        for (auto& b : m1) b = rnd();
        for (auto& b : pay) b = rnd();
        if (nx_host_respond(s, e, pro, pl, m1, 64 + l1, pay.data(), p2, msg2.data(), k1, k2, hh) != 1)
          return nfail("handshake", 1000 * pl + 10 * l1 + p2);
        ++runs;
        // the rejections: both length limits and a small-order key in each position
        for (int what = 0; what < 4; ++what) {
          uint8_t bad[160];
          std::memcpy(bad, m1, sizeof bad);
          if (what >= 2) std::memset(bad + 32 * (what - 2), 0, 32);
          const uint32_t len = what == 0 ? 63 : what == 1 ? 129 : 64 + l1;
          if (nx_host_respond(s, e, pro, pl, bad, len, pay.data(), p2, msg2.data(), k1, k2, hh) != 0)
            return nfail("rejection", what);
          uint32_t any = 0;
          for (uint32_t i = 0; i < 96 + p2; ++i) any |= msg2[i];
          for (int i = 0; i < 32; ++i) any |= k1[i] | k2[i] | hh[i] | hh[32 + i];
          if (any) return nfail("a rejected handshake's outputs are not zero", what);
        }
      }
  std::printf("noise_host ok: %d handshakes, 4 rejections each\n", runs);
  return 0;
}
#endif
