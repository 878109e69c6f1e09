// noise_init_host.cpp — the device Noise IX initiator (grapevine_amd/csrc/
// gvs_noise_init.h) built for the CPU: the four phases of k_noise_ixi stepped
// over four lane states, chained with x25519_quad_host and the serial ciphers
// the way gvs_noise_ix_initiate and gvs_noise_ix_finish chain the kernels.
// tests/test_noise_init.py checks it against grapevine_amd/noise.py without a
// GPU.  With -DNINIT_HOST_MAIN it is a program of its own that completes
// handshakes against the host responder of noise_host.cpp at the padding-edge
// lengths and runs the rejections (for a sanitizer build).  Test
// infrastructure only.
#include "noise_host.cpp"  // nx_host_respond, te0_table
#include "../grapevine_amd/csrc/gvs_chachapoly.h"
#include "../grapevine_amd/csrc/gvs_noise_init.h"

static void nxi_x(const uint8_t* sc, const uint8_t* pt, uint8_t* out, uint32_t* ok) {
  Fe r[4];
  x25519_quad_host(sc, pt, r);
  uint32_t any = 0;
  for (int i = 0; i < 32; ++i) any |= out[i] = (uint8_t)(r[0].v[i / 4] >> (8 * (i % 4)));
  if (ok) *ok = any != 0;
}

static bool nxi_open(uint32_t cipher, const uint8_t* key, const uint8_t* aad, const uint8_t* in, uint32_t len,
                     uint8_t* out) {
  const uint8_t iv[12] = {};
  return cipher ? gvs::chachapoly_item(false, key, iv, aad, 64, in, len, out)
                : gvs::aead_serial(false, te0_table(), key, iv, aad, 64, in, len, out);
}

extern "C" {

// -> e, s: msg1 holds 64 + pl bytes, state 64.  Returns 1, or -1 if lane states
// that hold the same value disagree.
int nxi_host_initiate(uint32_t cipher, const uint8_t* s, const uint8_t* e, const uint8_t* pro, uint32_t pro_len,
                      const uint8_t* payload, uint32_t pl, uint8_t* msg1, uint8_t* state) {
  std::vector<uint8_t> cell(64), xout(64);
  if (pro_len) std::memcpy(cell.data(), pro, pro_len);
  nxi_x(e, nullptr, xout.data(), nullptr);
  nxi_x(s, nullptr, xout.data() + 32, nullptr);
  uint32_t len1 = 0;
  NxiArgs a{};
  a.n = 1, a.pro = cell.data(), a.pro_len = pro_len, a.payload = pl ? payload : nullptr, a.payload_len = pl;
  a.msg1 = msg1, a.msg1_stride = 64 + pl, a.msg1_lens = &len1, a.states = state, a.xout = xout.data();
  const bool agree = cipher ? nxi_item_host<kNxiM1, true>(a, 0) : nxi_item_host<kNxiM1, false>(a, 0);
  return agree && len1 == 64 + pl ? 1 : -1;
}

// <- e, ee, se, s, es.  rs, k1, k2 32 bytes each, hh 64, payload2 `cap` bytes
// (written whole).  Returns the handshake's ok, or -1 for disagreeing lanes.
int nxi_host_finish(uint32_t cipher, const uint8_t* s, const uint8_t* e, const uint8_t* state, const uint8_t* msg2,
                    uint32_t msg2_len, uint8_t* rs, uint8_t* payload2, uint32_t cap, uint32_t* payload2_len,
                    uint8_t* k1, uint8_t* k2, uint8_t* hh) {
  const uint32_t stride = msg2_len > 96 ? msg2_len : 96, c2 = stride - 80;
  std::vector<uint8_t> slot(stride), st0(state, state + 64), xout(64), xout3(32), st(128), key(32), aad(64), pt1(32),
      pt2(c2);
  if (msg2_len) std::memcpy(slot.data(), msg2, msg2_len);
  uint32_t xok[2], xok3, ok1, ok2, ok = 0;
  NxiArgs a{};
  a.n = 1, a.states = st0.data(), a.xout = xout.data(), a.xok = xok, a.xout3 = xout3.data(), a.xok3 = &xok3;
  a.msg2 = slot.data(), a.msg2_stride = stride, a.msg2_lens = &msg2_len;
  a.st = st.data(), a.key = key.data(), a.aad = aad.data();
  a.ct1 = slot.data() + 32, a.ct2 = slot.data() + 80, a.ct2_stride = c2;
  a.pt1 = pt1.data(), a.pt2 = pt2.data(), a.pt2_stride = c2, a.ok1 = &ok1, a.ok2 = &ok2;
  a.rs = rs, a.payload2 = payload2, a.payload2_stride = cap, a.payload2_lens = payload2_len;
  a.send = k1, a.recv = k2, a.hashes = hh, a.ok = &ok;
  const bool len_ok = nxi_len_ok(a, msg2_len);
  nxi_x(e, slot.data(), xout.data(), &xok[0]);       // ee
  nxi_x(s, slot.data(), xout.data() + 32, &xok[1]);  // se
  bool agree = cipher ? nxi_item_host<kNxiA, true>(a, 0) : nxi_item_host<kNxiA, false>(a, 0);
  ok1 = nxi_open(cipher, key.data(), aad.data(), a.ct1, 48, pt1.data());
  nxi_x(e, pt1.data(), xout3.data(), &xok3);  // es: on zeros where ct_s did not open
  agree &= nxi_item_host<kNxiB, false>(a, 0);
  ok2 = len_ok && nxi_open(cipher, key.data(), aad.data(), a.ct2, msg2_len - 80, pt2.data());
  agree &= nxi_item_host<kNxiC, false>(a, 0);
  return agree ? (int)ok : -1;
}
}

#ifdef NINIT_HOST_MAIN
static int nifail(const char* what, unsigned at) {
  std::printf("noise_init_host: %s (%u)\n", what, at);
  return 1;
}

int main() {
  uint32_t x = 11;
  auto rnd = [&] { return (uint8_t)((x = x * 1664525u + 1013904223u) >> 24); };
  const uint32_t edge[2] = {0, 64}, p2s[6] = {0, 31, 32, 111, 112, 2048};
  uint8_t rsk[32], rek[32], s[32], e[32], pro[64], pay1[64], m1[128], state[64], rs[32], k1[32], k2[32], hh[64],
      r1[32], r2[32], rh[64], spub[32];
  std::vector<uint8_t> pay(2048), msg2(96 + 2048), got(2048);
  int runs = 0;
  for (uint32_t pl : edge)
    for (uint32_t l1 : edge)
      for (uint32_t p2 : p2s) {
        for (auto* v : {rsk, rek, s, e}) for (int i = 0; i < 32; ++i) v[i] = rnd();
        for (auto& b : pro) b = rnd();
        for (auto& b : pay1) b = rnd();
        for (auto& b : pay) b = rnd();
        uint32_t plen = 7;
        if (nxi_host_initiate(0, s, e, pro, pl, pay1, l1, m1, state) != 1) return nifail("initiate", 100 * pl + l1);
        if (nx_host_respond(rsk, rek, pro, pl, m1, 64 + l1, pay.data(), p2, msg2.data(), r1, r2, rh) != 1)
          return nifail("the responder refuses message 1", 100 * pl + l1);
        if (nxi_host_finish(0, s, e, state, msg2.data(), 96 + p2, rs, got.data(), 2048, &plen, k1, k2, hh) != 1)
          return nifail("finish", p2);
        nxi_x(rsk, nullptr, spub, nullptr);
        if (plen != p2 || std::memcmp(got.data(), pay.data(), p2) || std::memcmp(rs, spub, 32) ||
            std::memcmp(k1, r1, 32) || std::memcmp(k2, r2, 32) || std::memcmp(hh, rh, 64))
          return nifail("the two sides disagree", p2);
        ++runs;
        // the rejections: ct_s, ct_p's tag, a short message, a small-order re; ChaChaPoly opens nothing sealed by AES-GCM
        for (int what = 0; what < 5; ++what) {
          std::vector<uint8_t> bad(msg2.begin(), msg2.begin() + 96 + p2);
          if (what == 0) bad[40] ^= 1;
          if (what == 1) bad[95 + p2] ^= 0x80;
          if (what == 3) std::memset(bad.data(), 0, 32);
          const uint32_t len = what == 2 ? 95 : 96 + p2;
          if (nxi_host_finish(what == 4, s, e, state, bad.data(), len, rs, got.data(), 2048, &plen, k1, k2, hh) != 0)
            return nifail("rejection", what);
          uint32_t any = plen;
          for (uint32_t i = 0; i < 2048; ++i) any |= got[i];
          for (int i = 0; i < 32; ++i) any |= rs[i] | k1[i] | k2[i] | hh[i] | hh[32 + i];
          if (any) return nifail("a rejected handshake's outputs are not zero", what);
        }
      }
  if (nxi_host_initiate(1, s, e, pro, 64, pay1, 64, m1, state) != 1) return nifail("initiate, ChaChaPoly", 0);
  std::printf("noise_init_host ok: %d handshakes, 5 rejections each\n", runs);
  return 0;
}
#endif
