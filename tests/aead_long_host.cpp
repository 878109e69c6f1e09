// aead_long_host.cpp — the long channel cipher's schedule
// (grapevine_amd/csrc/gvs_aead_long.h: the distance map, the power table, the
// Horner tiles, the slot products, the tag and the open path's masked second
// pass) built for the CPU: 256 thread states are stepped through the phases
// that the kernel's barriers separate, over an array that stands for the
// workgroup's cells.  tests/test_aead_long.py checks it against the Python
// reference.  With -DAEAD_LONG_HOST_MAIN it is a stand-alone program (round
// trips against the serial form of gvs_aead.h and two rejections at each
// length), which is what a sanitizer build runs.  Test infrastructure only.
#include "aead_host.cpp"
#include "../grapevine_amd/csrc/gvs_aead_long.h"

// One message through the schedule.  seal: in = P (in_len B), out = C | tag.
// open: in = C | tag, out = P, or zeros and false.  `out` holds the rounded-up
// text and, sealing, the tag.
static bool aead_long_sched(bool seal, const uint8_t key[32], const uint8_t ivb[12], const uint8_t* aad_b,
                            uint32_t aad_len, const uint8_t* in_b, uint32_t in_len, uint8_t* out_b) {
  if (!seal && in_len < kAeadTag) return false;
  const uint32_t* te0 = te0_table();
  const AlShape s = al_shape(seal ? in_len : in_len - kAeadTag, aad_len);
  // block-aligned copies: the schedule moves whole 16-byte blocks
  std::vector<uint4> aad(kAeadAadMax / 16), in(s.nc + 2), out(s.nc + 2), cells(kAlCells);
  if (aad_len) std::memcpy(aad.data(), aad_b, aad_len);
  if (in_len) std::memcpy(in.data(), in_b, in_len);
  const uint8_t *aadp = (const uint8_t*)aad.data(), *inp = (const uint8_t*)in.data();
  uint8_t* outp = (uint8_t*)out.data();

  // 1. the key schedule, H and E_K(IV | 1)
  uint32_t kw[8], w[60];
  for (int i = 0; i < 8; ++i) kw[i] = ae_be32(key + 4 * i);
  aes256_expand(te0, kw, w);
  for (int r = 0; r < 15; ++r) cells[kAlRk + r] = make_uint4(w[4 * r], w[4 * r + 1], w[4 * r + 2], w[4 * r + 3]);
  const uint4* rk = cells.data() + kAlRk;
  uint4* hp = cells.data() + kAlHp;
  const uint32_t iv[3] = {ae_be32(ivb), ae_be32(ivb + 4), ae_be32(ivb + 8)};
  uint32_t hb[4] = {0, 0, 0, 0}, ej[4] = {iv[0], iv[1], iv[2], 1u};
  aes256_encrypt2(rk, te0, hb, ej);
  hp[0] = make_uint4(hb[3], hb[2], hb[1], hb[0]);
  cells[kAlEj] = make_uint4(ej[0], ej[1], ej[2], ej[3]);

  // 2. the powers: a barrier after every step
  for (uint32_t step = 1; step < s.maxp; step <<= 1)
    for (uint32_t t = 0; t < kAlThreads; ++t) al_pow_step(hp, step, t);
  const Gf128 ht = al_gf(hp[s.m > kAlT ? kAlT - 1u : 0u]);

  // 3, 4. every thread's tiles and its share of S
  Gf128 sum{{0, 0, 0, 0}};
  for (uint32_t t = 0; t < kAlThreads; ++t) {
    Gf128 y[2] = {{{0, 0, 0, 0}}, {{0, 0, 0, 0}}};
    for (uint32_t k = s.ntile; k-- > 0;) {
      if (seal)
        al_tile<true>(s, rk, te0, iv, aadp, inp, outp, k, t, k + 1u == s.ntile, ht, y);
      else
        al_tile<false>(s, rk, te0, iv, aadp, inp, outp, k, t, k + 1u == s.ntile, ht, y);
    }
    const Gf128 p = al_final(s, hp, t, t & ~63u, y);
    for (int q = 0; q < 4; ++q) sum.w[q] ^= p.w[q];
  }

  // 5. the tag; open: the verdict, then the masked second pass
  uint32_t differs = 0;
  for (uint32_t b = 0; b < 16; ++b) {
    const uint32_t tb = al_tag_byte(sum, cells[kAlEj], b);
    if (seal)
      out_b[s.text_len + b] = (uint8_t)tb;
    else
      differs |= tb ^ inp[s.text_len + b];
  }
  if (!seal)
    for (uint32_t t = 0; t < kAlThreads; ++t)
      for (uint32_t k = 0; k < (s.nc + kAlT - 1u) / kAlT; ++k)
        al_open_tile(s, rk, te0, iv, inp, outp, k, t, differs ? 0u : ~0u);
  if (s.text_len) std::memcpy(out_b, outp, s.text_len);
  return differs == 0;
}

extern "C" {

// out (len + 16 B) = C | tag
void aead_long_host_seal(const uint8_t* key, const uint8_t* iv, const uint8_t* aad, uint32_t aad_len,
                         const uint8_t* pt, uint32_t len, uint8_t* out) {
  aead_long_sched(true, key, iv, aad, aad_len, pt, len, out);
}

// in = C | tag (len B); out (len - 16 B) = P; returns 1, or 0 with out zeroed
int aead_long_host_open(const uint8_t* key, const uint8_t* iv, const uint8_t* aad, uint32_t aad_len,
                        const uint8_t* in, uint32_t len, uint8_t* out) {
  return aead_long_sched(false, key, iv, aad, aad_len, in, len, out) ? 1 : 0;
}
}

#ifdef AEAD_LONG_HOST_MAIN
static int fail(const char* what, unsigned at) {
  std::printf("aead_long_host: %s (%u)\n", what, at);
  return 1;
}

// the lengths of tests/test_aead_long.py: block edges, the short path's limit,
// the hash-block counts around one and two strides, the maximum
int main() {
  std::vector<std::pair<uint32_t, uint32_t>> cases;  // (text length, AAD length)
  for (uint32_t aad_len : {0u, 20u, 64u}) {
    for (uint32_t len : {0u, 1u, 16u, 2048u, 2049u, kAeadLongTextMax}) cases.push_back({len, aad_len});
    for (uint32_t j = 1; j <= 2; ++j)
      for (int dm = -1; dm <= 1; ++dm)
        for (uint32_t last : {16u, 1u, 15u})  // m = na + nc + 1 = j kAlT + dm
          cases.push_back({(j * kAlT + dm - 1 - (aad_len + 15) / 16 - 1) * 16 + last, aad_len});
  }
  uint32_t x = 7;
  auto rnd = [&] { return (uint8_t)((x = x * 1664525u + 1013904223u) >> 24); };
  for (const auto& cs : cases) {
    const uint32_t len = cs.first, aad_len = cs.second;
    std::vector<uint8_t> key(32), iv(12), aad(aad_len), pt(len), ct(len + 16), want(len + 16), back(len);
    for (auto* v : {&key, &iv, &aad, &pt})
      for (auto& b : *v) b = rnd();
    aead_long_host_seal(key.data(), iv.data(), aad.data(), aad_len, pt.data(), len, ct.data());
    aead_host_seal(key.data(), iv.data(), aad.data(), aad_len, pt.data(), len, want.data());
    if (ct != want) return fail("seal differs from the serial form", len);
    if (!aead_long_host_open(key.data(), iv.data(), aad.data(), aad_len, ct.data(), len + 16, back.data()) || back != pt)
      return fail("round trip", len);
    for (uint32_t spoil : {len / 2, len + 15}) {  // a ciphertext byte (the tag's first if there is none), a tag byte
      ct[spoil] ^= 0x10;
      if (aead_long_host_open(key.data(), iv.data(), aad.data(), aad_len, ct.data(), len + 16, back.data()) ||
          back != std::vector<uint8_t>(len))
        return fail("rejection", len);
      ct[spoil] ^= 0x10;
    }
  }
  std::printf("aead_long_host ok: %zu cases\n", cases.size());
  return 0;
}
#endif
