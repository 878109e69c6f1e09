// chachapoly_long_host.cpp — the long ChaCha20-Poly1305 schedule
// (grapevine_amd/csrc/gvs_chachapoly_long.h: the chunk grid, the power steps,
// the Horner tiles, the final exponents, the fold's carries and the open
// path's masked second pass) built for the CPU: 256 thread states are stepped
// through the phases that the kernel's barriers separate, over an array that
// stands for the workgroup's words.  tests/test_chachapoly_long.py checks it
// against the Python reference.  With -DCHACHAPOLY_LONG_HOST_MAIN it is a
// stand-alone program (round trips against the serial form of
// gvs_chachapoly.h and two rejections at each length), which is what a
// sanitizer build runs.  Test infrastructure only.
#include "../grapevine_amd/csrc/gvs_chachapoly_long.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace gvs;

// phases 2 and 4 of the kernel around `tiles(t, R, y)`, which runs thread t's
// tiles: w holds r at entry 0 of the power table; returns the tag under s
template <typename Tiles>
static void cl_mac(const ClShape& s, std::vector<uint32_t>& w, const uint32_t sw[4], Tiles&& tiles, uint32_t tg[4]) {
  for (uint32_t step = 1; step < s.maxp; step <<= 1)  // a barrier after every step
    for (uint32_t t = 0; t < kClThreads; ++t) cl_pow_step(w.data(), step, s.maxp, t);
  const P130 R = cl_pw_get(w.data(), s.end > kClT ? kClT - 1u : 0u);
  P130 h{{0, 0, 0, 0, 0}};
  for (uint32_t wave = 0; wave < kClThreads / 64; ++wave) {
    P130 q{{0, 0, 0, 0, 0}};
    for (uint32_t g = 0; g < 4; ++g) {  // the butterfly: 16 lanes, a carry pass, then the four groups
      P130 p{{0, 0, 0, 0, 0}};
      for (uint32_t l = 0; l < 16; ++l) {
        const uint32_t t = 64 * wave + 16 * g + l;
        P130 y[4] = {};
        tiles(t, R, y);
        p = p130_add(p, cl_final(s, w.data(), t, 64 * wave, y));
      }
      p130_carry(p);
      q = p130_add(q, p);
    }
    h = p130_add(h, q);
  }
  p130_finish(h, sw, tg);
}

// One message through the schedule.  seal: in = P (in_len B), out = C | tag.
// open: in = C | tag, out = P, or zeros and false.
static bool cl_sched(bool seal, const uint8_t key[32], const uint8_t nonce[12], const uint8_t* aad_b, uint32_t aad_len,
                     const uint8_t* in_b, uint32_t in_len, uint8_t* out_b) {
  if (!seal && in_len < kAeadTag) return false;
  const ClShape s = cl_shape(seal ? in_len : in_len - kAeadTag, aad_len);
  // block-aligned copies: the schedule moves whole 16-byte blocks
  std::vector<uint4> aad(kAeadAadMax / 16), in(s.nc + 2), out(s.nc + 2);
  std::vector<uint32_t> w(kClWords);
  if (aad_len) std::memcpy(aad.data(), aad_b, aad_len);
  if (in_len) std::memcpy(in.data(), in_b, in_len);
  const uint8_t *aadp = (const uint8_t*)aad.data(), *inp = (const uint8_t*)in.data();
  uint8_t* outp = (uint8_t*)out.data();
  uint32_t kw[8], nw[3], ks0[16], tg[4];
  for (int k = 0; k < 8; ++k) kw[k] = cp_le32(key + 4 * k);
  for (int k = 0; k < 3; ++k) nw[k] = cp_le32(nonce + 4 * k);

  // 1. thread 0's block is the one-time key
  cp_block(kw, 0, nw, ks0);
  cl_pw_put(w.data(), 0, p130_clamp_r(ks0));

  // 2 .. 4. the powers, every thread's tiles and the fold
  cl_mac(s, w, ks0 + 4, [&](uint32_t t, const P130& R, P130 (&y)[4]) {
    for (uint32_t k = 0; k < s.ntile; ++k) {
      const uint32_t Q = kClThreads * k + t;
      if (4u * (kClThreads * k + (t & ~63u)) >= s.end) continue;
      uint32_t ks[16];
      cp_block(kw, Q, nw, ks);
      if (seal)
        cl_tile<true>(s, ks, aadp, inp, outp, Q, k == 0, R, y);
      else
        cl_tile<false>(s, ks, aadp, inp, outp, Q, k == 0, R, y);
    }
  }, tg);

  // 5. the tag; open: the verdict, then the masked second pass
  uint32_t differs = 0;
  for (uint32_t b = 0; b < 16; ++b) {
    if (seal)
      out_b[s.text_len + b] = (uint8_t)cl_tag_byte(tg, b);
    else
      differs |= cl_tag_byte(tg, b) ^ inp[s.text_len + b];
  }
  if (!seal && s.nc)
    for (uint32_t Q = 0; Q < (s.nc + 3u) / 4u + 1u; ++Q) {
      uint32_t ks[16];
      cp_block(kw, Q, nw, ks);
      cl_open_tile(s, ks, inp, outp, Q, differs ? 0u : ~0u);
    }
  if (s.text_len) std::memcpy(out_b, outp, s.text_len);
  return differs == 0;
}

extern "C" {

// out (len + 16 B) = C | tag
void chachapoly_long_host_seal(const uint8_t* key, const uint8_t* nonce, const uint8_t* aad, uint32_t aad_len,
                               const uint8_t* pt, uint32_t len, uint8_t* out) {
  cl_sched(true, key, nonce, aad, aad_len, pt, len, out);
}

// in = C | tag (len B); out (len - 16 B) = P; returns 1, or 0 with out zeroed
int chachapoly_long_host_open(const uint8_t* key, const uint8_t* nonce, const uint8_t* aad, uint32_t aad_len,
                              const uint8_t* in, uint32_t len, uint8_t* out) {
  return cl_sched(false, key, nonce, aad, aad_len, in, len, out) ? 1 : 0;
}

// tag (16 B) = Poly1305 under the one-time key (32 B: any r, clamped here) of
// nblk whole 16-byte blocks, laid on the grid from cell 4 on
void chachapoly_long_host_poly1305(const uint8_t* key, const uint8_t* blocks, uint32_t nblk, uint8_t* tag) {
  const ClShape s = cl_grid(4u, 4u + nblk);
  std::vector<uint32_t> w(kClWords);
  uint32_t rw[4], sw[4], tg[4];
  for (int k = 0; k < 4; ++k) rw[k] = cp_le32(key + 4 * k), sw[k] = cp_le32(key + 16 + 4 * k);
  cl_pw_put(w.data(), 0, p130_clamp_r(rw));
  cl_mac(s, w, sw, [&](uint32_t t, const P130& R, P130 (&y)[4]) {
    for (uint32_t k = 0; k < s.ntile; ++k)
      for (uint32_t u = 0; u < 4; ++u) {
        const uint32_t p = 4u * (kClThreads * k + t) + u;
        const uint8_t* b = blocks + (p >= 4u && p < s.end ? 16u * (size_t)(p - 4u) : 0u);  // a cell outside the grid is not absorbed
        const uint4 x = make_uint4(cp_le32(b), cp_le32(b + 4), cp_le32(b + 8), cp_le32(b + 12));
        cl_absorb(s, p, x, k == 0, R, y[u]);
      }
  }, tg);
  for (uint32_t k = 0; k < 16; ++k) tag[k] = (uint8_t)cl_tag_byte(tg, k);
}
}

#ifdef CHACHAPOLY_LONG_HOST_MAIN
static int fail(const char* what, unsigned at) {
  std::printf("chachapoly_long_host: %s (%u)\n", what, at);
  return 1;
}

// the lengths of tests/test_chachapoly_long.py: block and chunk edges, the
// short path's limit, the grid's end around one, two and four strides, the
// maximum; then Poly1305 alone with every bit of r set before the clamp
int main() {
  std::vector<std::pair<uint32_t, uint32_t>> cases;  // (text length, AAD length)
  for (uint32_t aad_len : {0u, 20u, 64u}) {
    for (uint32_t len : {0u, 1u, 16u, 63u, 64u, 65u, 2048u, 2049u, kAeadLongTextMax}) cases.push_back({len, aad_len});
    for (uint32_t j : {1u, 2u, 4u})
      for (int de = -1; de <= 1; ++de)
        for (uint32_t last : {16u, 1u, 15u})  // E = nc + 5 = j kClT + de
          cases.push_back({(j * kClT + de - 6) * 16 + last, aad_len});
  }
  uint32_t x = 7;
  auto rnd = [&] { return (uint8_t)((x = x * 1664525u + 1013904223u) >> 24); };
  for (const auto& cs : cases) {
    const uint32_t len = cs.first, aad_len = cs.second;
    std::vector<uint8_t> key(32), nonce(12), aad(aad_len), pt(len), ct(len + 16), want(len + 16), back(len);
    for (auto* v : {&key, &nonce, &aad, &pt})
      for (auto& b : *v) b = rnd();
    chachapoly_long_host_seal(key.data(), nonce.data(), aad.data(), aad_len, pt.data(), len, ct.data());
    chachapoly_item(true, key.data(), nonce.data(), aad.data(), aad_len, pt.data(), len, want.data());
    if (ct != want) return fail("seal differs from the serial form", len);
    if (!chachapoly_long_host_open(key.data(), nonce.data(), aad.data(), aad_len, ct.data(), len + 16, back.data()) ||
        back != pt)
      return fail("round trip", len);
    for (uint32_t spoil : {len / 2, len + 15}) {  // a ciphertext byte (the tag's first if there is none), a tag byte
      ct[spoil] ^= 0x10;
      if (chachapoly_long_host_open(key.data(), nonce.data(), aad.data(), aad_len, ct.data(), len + 16, back.data()) ||
          back != std::vector<uint8_t>(len))
        return fail("rejection", len);
      ct[spoil] ^= 0x10;
    }
  }
  const uint32_t nblk = 2 * kClT + 3;
  std::vector<uint8_t> otk(32, 0xff), blocks(16 * nblk, 0xff);
  uint8_t tag[16], want[16];
  chachapoly_long_host_poly1305(otk.data(), blocks.data(), nblk, tag);
  poly1305(otk.data(), blocks.data(), blocks.size(), want);
  if (std::memcmp(tag, want, 16)) return fail("Poly1305 with r all ones", nblk);
  std::printf("chachapoly_long_host ok: %zu cases\n", cases.size());
  return 0;
}
#endif
