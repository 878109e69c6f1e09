// gvs_chachapoly.h — the attested channel's second cipher on the device:
// ChaCha20-Poly1305 (RFC 8439 §2.8), Noise's ChaChaPoly, batched over messages
// that each have a key and a nonce of their own.  Per message:
//   otk  = ChaCha20(key, counter 0, nonce)[0:32]          r (clamped) | s
//   C    = P ^ ChaCha20(key, counter 1.., nonce)
//   tag  = Poly1305_r,s(pad16(AAD) | pad16(C) | le64(|AAD|) | le64(|C|))
// Only 32-bit add, rotate and xor, and 130-bit multiplies from 32 x 32 -> 64
// products: no table, and no address that follows a key or the text.
//
// The primitives (the block function with RFC 8439's counter and nonce, the
// Poly1305 multiply, carry and finish over five 26-bit limbs, a serial
// whole-message form) are host/device code, so tests/chachapoly_host.cpp runs
// them on the CPU.  The kernel, k_chachapoly<SEAL>, is their row form: one DPP
// row (16 lanes) per message.
//
// What depends on data: loop trip counts follow a message's length and AAD
// length, which the caller passes in clear; rows of one wave with different
// lengths are masked.  Keys, nonces, text, r, s and the outcome of the tag
// comparison reach no branch and no address.  A message that fails is zeroed
// through selects; its stores are the stores of one that passes.
#pragma once
#include "gvs_aead.h"
#include "gvs_chacha_rounds.h"

namespace gvs {

#define GVS_CP_FN __host__ __device__ __attribute__((always_inline)) inline

constexpr uint32_t kCpRow = 16;                // lanes per message
constexpr uint32_t kCpMsgs = 16;               // messages per workgroup
constexpr uint32_t kCpThreads = kCpRow * kCpMsgs;
// a message's MAC input in 16-byte cells: AAD, ciphertext, the length block
constexpr uint32_t kCpCells = kAeadAadMax / 16 + kAeadTextMax / 16 + 1;

// ------------------------------------------------------------------ ChaCha20

// out = the 64-byte block (16 little-endian words) of RFC 8439 §2.3: words
// 0..3 the constants, 4..11 the key, 12 the 32-bit block counter, 13..15 the
// 96-bit nonce
GVS_CP_FN void cp_block(const uint32_t key[8], uint32_t counter, const uint32_t nonce[3], uint32_t out[16]) {
  const uint32_t c0 = 0x61707865u, c1 = 0x3320646eu, c2 = 0x79622d32u, c3 = 0x6b206574u;
  uint32_t x0 = c0, x1 = c1, x2 = c2, x3 = c3;
  uint32_t x4 = key[0], x5 = key[1], x6 = key[2], x7 = key[3];
  uint32_t x8 = key[4], x9 = key[5], x10 = key[6], x11 = key[7];
  uint32_t x12 = counter, x13 = nonce[0], x14 = nonce[1], x15 = nonce[2];
  GVS_CC_ROUNDS20
  out[0] = x0 + c0, out[1] = x1 + c1, out[2] = x2 + c2, out[3] = x3 + c3;
  out[4] = x4 + key[0], out[5] = x5 + key[1], out[6] = x6 + key[2], out[7] = x7 + key[3];
  out[8] = x8 + key[4], out[9] = x9 + key[5], out[10] = x10 + key[6], out[11] = x11 + key[7];
  out[12] = x12 + counter, out[13] = x13 + nonce[0], out[14] = x14 + nonce[1], out[15] = x15 + nonce[2];
}

// ------------------------------------------------------------------ Poly1305

// An integer mod 2^130 - 5 as five 26-bit limbs, v[0] the least significant.
// "Carried" below: every limb below 2^26 + 2^9.
struct P130 {
  uint32_t v[5];
};
constexpr uint32_t kP26 = 0x3ffffffu;

// the 16 bytes of a block as four little-endian words, plus hibit * 2^128
GVS_CP_FN P130 p130_of_block(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t hibit) {
  return P130{{w0 & kP26, ((w0 >> 26) | (w1 << 6)) & kP26, ((w1 >> 20) | (w2 << 12)) & kP26,
               ((w2 >> 14) | (w3 << 18)) & kP26, (w3 >> 8) | (hibit << 24)}};
}

// r of a one-time key's first four words, clamped (RFC 8439 §2.5)
GVS_CP_FN P130 p130_clamp_r(const uint32_t w[4]) {
  return p130_of_block(w[0] & 0x0fffffffu, w[1] & 0x0ffffffcu, w[2] & 0x0ffffffcu, w[3] & 0x0ffffffcu, 0);
}

GVS_CP_FN P130 p130_add(const P130& a, const P130& b) {
  return P130{{a.v[0] + b.v[0], a.v[1] + b.v[1], a.v[2] + b.v[2], a.v[3] + b.v[3], a.v[4] + b.v[4]}};
}

// a * b mod 2^130 - 5, carried.  a: limbs below 2^27 + 2^10 (a carried value
// plus a block); b: carried.  25 products (v_mad_u64_u32 on the device)
// against b and 5 b: a limb of 5 b is below 2^28.4, a column of five products
// below 2^57.8.  The carries stay 64 bits wide: the top limb's is below 2^32,
// and five times that is not a 32-bit number.
GVS_CP_FN P130 p130_mul(const P130& a, const P130& b) {
  const uint32_t a0 = a.v[0], a1 = a.v[1], a2 = a.v[2], a3 = a.v[3], a4 = a.v[4];
  const uint32_t b0 = b.v[0], b1 = b.v[1], b2 = b.v[2], b3 = b.v[3], b4 = b.v[4];
  const uint32_t s1 = b1 * 5u, s2 = b2 * 5u, s3 = b3 * 5u, s4 = b4 * 5u;
  uint64_t d0 = (uint64_t)a0 * b0 + (uint64_t)a1 * s4 + (uint64_t)a2 * s3 + (uint64_t)a3 * s2 + (uint64_t)a4 * s1;
  uint64_t d1 = (uint64_t)a0 * b1 + (uint64_t)a1 * b0 + (uint64_t)a2 * s4 + (uint64_t)a3 * s3 + (uint64_t)a4 * s2;
  uint64_t d2 = (uint64_t)a0 * b2 + (uint64_t)a1 * b1 + (uint64_t)a2 * b0 + (uint64_t)a3 * s4 + (uint64_t)a4 * s3;
  uint64_t d3 = (uint64_t)a0 * b3 + (uint64_t)a1 * b2 + (uint64_t)a2 * b1 + (uint64_t)a3 * b0 + (uint64_t)a4 * s4;
  uint64_t d4 = (uint64_t)a0 * b4 + (uint64_t)a1 * b3 + (uint64_t)a2 * b2 + (uint64_t)a3 * b1 + (uint64_t)a4 * b0;
  d1 += d0 >> 26;
  d2 += d1 >> 26;
  d3 += d2 >> 26;
  d4 += d3 >> 26;
  const uint64_t t = (d0 & kP26) + (d4 >> 26) * 5u;  // below 2^26 + 5 * 2^32
  return P130{{(uint32_t)t & kP26, ((uint32_t)d1 & kP26) + (uint32_t)(t >> 26), (uint32_t)d2 & kP26,
               (uint32_t)d3 & kP26, (uint32_t)d4 & kP26}};
}

// one carry pass over limbs below 2^31: afterwards v[0], v[2..4] < 2^26 and
// v[1] <= 2^26
GVS_CP_FN void p130_carry(P130& h) {
  uint32_t c = h.v[0] >> 26;
  h.v[0] &= kP26;
#pragma unroll
  for (int k = 1; k < 5; ++k) {
    h.v[k] += c;
    c = h.v[k] >> 26;
    h.v[k] &= kP26;
  }
  h.v[0] += c * 5u;
  c = h.v[0] >> 26;
  h.v[0] &= kP26;
  h.v[1] += c;
}

// tag = ((h mod 2^130 - 5) + s) mod 2^128 as four little-endian words.  h:
// limbs below 2^31 (a sum of 16 carried values is).  Two passes carry h fully;
// h - p is taken by a select on the borrow, never a branch.
GVS_CP_FN void p130_finish(P130 h, const uint32_t s[4], uint32_t tag[4]) {
  p130_carry(h);
  p130_carry(h);
  uint32_t g[5], c = 5;  // g = h + 5 - 2^130
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    g[k] = h.v[k] + c;
    c = g[k] >> 26;
    g[k] &= kP26;
  }
  const uint32_t ge = 0u - c;  // all ones: h + 5 reached 2^130, so h >= p
#pragma unroll
  for (int k = 0; k < 5; ++k) h.v[k] = (g[k] & ge) | (h.v[k] & ~ge);
  const uint32_t w[4] = {h.v[0] | (h.v[1] << 26), (h.v[1] >> 6) | (h.v[2] << 20), (h.v[2] >> 12) | (h.v[3] << 14),
                         (h.v[3] >> 18) | (h.v[4] << 8)};
  uint64_t f = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    f += (uint64_t)w[k] + s[k];
    tag[k] = (uint32_t)f;
    f >>= 32;
  }
}

// ------------------------------------------------------------------ serial form

inline uint32_t cp_le32(const uint8_t* p) {
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// Poly1305 of any byte string on the host, block after block (RFC 8439 §2.5):
// the only place with a partial last block, which the AEAD never has
inline void poly1305(const uint8_t key[32], const uint8_t* msg, size_t len, uint8_t tag[16]) {
  uint32_t rw[4], sw[4], tw[4];
  for (int k = 0; k < 4; ++k) rw[k] = cp_le32(key + 4 * k), sw[k] = cp_le32(key + 16 + 4 * k);
  const P130 r = p130_clamp_r(rw);
  P130 h{{0, 0, 0, 0, 0}};
  for (size_t o = 0; o < len; o += 16) {
    uint8_t blk[16] = {};
    const size_t nb = len - o < 16 ? len - o : 16;
    for (size_t k = 0; k < nb; ++k) blk[k] = msg[o + k];
    if (nb < 16) blk[nb] = 1;
    h = p130_mul(p130_add(h, p130_of_block(cp_le32(blk), cp_le32(blk + 4), cp_le32(blk + 8), cp_le32(blk + 12),
                                           nb == 16 ? 1u : 0u)), r);
  }
  p130_finish(h, sw, tw);
  for (int k = 0; k < 16; ++k) tag[k] = (uint8_t)(tw[k >> 2] >> (8 * (k & 3)));
}

// One message on the host from the same primitives: the checker of the row
// form and what the CPU tests run.  seal: out = C | tag (in_len + 16 bytes),
// returns true.  open: in = C | tag; out = P (in_len - 16 bytes); a short
// message or a wrong tag returns false and zeroes out.
inline bool chachapoly_item(bool seal, const uint8_t key[32], const uint8_t nonce[12], const uint8_t* aad,
                            uint32_t aad_len, const uint8_t* in, uint32_t in_len, uint8_t* out) {
  if (!seal && in_len < kAeadTag) return false;
  const uint32_t len = seal ? in_len : in_len - kAeadTag;
  uint32_t kw[8], nw[3], ks[16], rw[4], sw[4], tw[4];
  for (int k = 0; k < 8; ++k) kw[k] = cp_le32(key + 4 * k);
  for (int k = 0; k < 3; ++k) nw[k] = cp_le32(nonce + 4 * k);
  cp_block(kw, 0, nw, ks);
  for (int k = 0; k < 4; ++k) rw[k] = ks[k], sw[k] = ks[4 + k];
  const P130 r = p130_clamp_r(rw);
  P130 h{{0, 0, 0, 0, 0}};
  auto absorb = [&](const uint8_t* p, uint32_t n) {  // n bytes, the last block zero-padded
    for (uint32_t o = 0; o < n; o += 16) {
      uint8_t blk[16] = {};
      for (uint32_t k = 0; k < 16 && o + k < n; ++k) blk[k] = p[o + k];
      h = p130_mul(p130_add(h, p130_of_block(cp_le32(blk), cp_le32(blk + 4), cp_le32(blk + 8), cp_le32(blk + 12), 1)), r);
    }
  };
  absorb(aad, aad_len);
  if (!seal) absorb(in, len);
  for (uint32_t o = 0; o < len; o += 64) {
    cp_block(kw, o / 64 + 1, nw, ks);
    for (uint32_t k = 0; k < 64 && o + k < len; ++k) out[o + k] = in[o + k] ^ (uint8_t)(ks[k >> 2] >> (8 * (k & 3)));
  }
  if (seal) absorb(out, len);
  h = p130_mul(p130_add(h, p130_of_block(aad_len, 0, len, 0, 1)), r);
  p130_finish(h, sw, tw);
  uint8_t tag[16];
  for (int k = 0; k < 16; ++k) tag[k] = (uint8_t)(tw[k >> 2] >> (8 * (k & 3)));
  if (seal) {
    for (int k = 0; k < 16; ++k) out[len + k] = tag[k];
    return true;
  }
  uint32_t diff = 0;
  for (int k = 0; k < 16; ++k) diff |= (uint32_t)(tag[k] ^ in[len + k]);
  for (uint32_t k = 0; k < len; ++k) out[k] = diff ? 0 : out[k];
  return diff == 0;
}

// ------------------------------------------------------------------ the kernel

#if defined(__HIPCC__)

// lane `src` of the row's value
__device__ inline P130 cp_row_get(const P130& p, uint32_t src) {
  P130 o;
#pragma unroll
  for (int k = 0; k < 5; ++k) o.v[k] = __shfl(p.v[k], (int)src, (int)kCpRow);
  return o;
}

// One row of 16 lanes per message (lane j below), four messages per wave, 16
// per workgroup; the grid follows n only.  The arguments are k_aead's
// (AeadArgs; `te` is not read).
//  1. the MAC input goes to the row's 133 LDS cells at its Poly1305 position:
//     the AAD blocks, the length block and, on open, the received ciphertext
//  2. ChaCha20 pass p gives lane j block 16 p + j.  Block 0 (lane 0, pass 0)
//     is the one-time key, broadcast over the row; block c >= 1 is XORed over
//     text bytes [64 (c - 1), 64 c).  Seal runs its passes here, writing the
//     ciphertext to `out` and to LDS; open keeps pass 0's block in registers
//     and runs its passes after the verdict, so that what it stores is
//     text & verdict
//  3. r^(j + 1) by four log-step doubling rounds (round s gives lanes
//     [s, 2 s) r^s * r^(j + 1 - s)); R = r^16 is lane 15's
//  4. Poly1305 over blocks counted from the end, e = M - 1 - i: lane j runs
//     Horner with R over the blocks e = j (mod 16), then multiplies by
//     r^(j + 1); four butterflies sum the 16 carried values limb by limb
//     (below 2^31), and p130_finish carries, reduces and adds s
//  5. open: the tag is compared bytewise, lane j byte j, and OR-folded over
//     the row; every block of the output slot is stored, zero past the text
template <bool SEAL>
__global__ void __launch_bounds__(kCpThreads) k_chachapoly(AeadArgs a) {
  __shared__ uint4 s_x[kCpMsgs * kCpCells];
  const uint32_t j = threadIdx.x & (kCpRow - 1u);
  const uint32_t row = threadIdx.x / kCpRow;
  const uint32_t i = blockIdx.x * kCpMsgs + row;
  if (i >= a.n) return;  // whole rows: no lane of a live row waits for them
  uint4* const X = s_x + row * kCpCells;

  // lengths: per row, and the only data that loops and addresses follow
  const uint32_t in_len = a.in_lens[i];
  uint32_t aad_len = a.aad ? a.aad_lens[i] : 0u;
  const bool merge = SEAL && a.opened != nullptr;
  bool len_ok = (in_len <= a.in_stride) & (aad_len <= kAeadAadMax) & (aad_len <= a.aad_stride);
  uint32_t text_len;
  if (SEAL) {
    text_len = in_len;
    len_ok = len_ok & (text_len <= kAeadTextMax) & ((uint64_t)text_len + kAeadTag <= a.out_stride);
    if (merge) len_ok = len_ok & (text_len != 0);  // an empty response is not sealed
  } else {
    len_ok = len_ok & (in_len >= kAeadTag);
    text_len = in_len - kAeadTag;
    len_ok = len_ok & (text_len <= kAeadTextMax) & (text_len <= a.out_stride);
  }
  text_len = len_ok ? text_len : 0u;
  aad_len = len_ok ? aad_len : 0u;
  const uint32_t nc = (text_len + 15u) / 16u, na = (aad_len + 15u) / 16u;
  const uint32_t m = na + nc + 1u;            // MAC blocks, <= kCpCells
  const uint32_t nb64 = (text_len + 63u) / 64u;  // keystream blocks 1 .. nb64

  // 1. the MAC input
  const uint8_t* inp = a.in + (uint64_t)i * a.in_stride;
  uint8_t* outp = a.out + (uint64_t)i * a.out_stride;
  if (j < na) {
    const uint4 d = *reinterpret_cast<const uint4*>(a.aad + (uint64_t)i * a.aad_stride + 16u * j);
    X[j] = ae_keep(d, (int)aad_len - 16 * (int)j);
  }
  if (j == 0) X[na + nc] = make_uint4(aad_len, 0u, text_len, 0u);
  if (!SEAL) {
    for (uint32_t t = j; t < nc; t += kCpRow)
      X[na + t] = ae_keep(*reinterpret_cast<const uint4*>(inp + 16u * t), (int)text_len - 16 * (int)t);
  }

  // 2. ChaCha20
  const uint4 k0 = a.keys[2 * (uint64_t)i], k1 = a.keys[2 * (uint64_t)i + 1];
  const uint32_t key[8] = {k0.x, k0.y, k0.z, k0.w, k1.x, k1.y, k1.z, k1.w};
  const uint32_t* np = a.ivs + 3 * (uint64_t)i;
  const uint32_t nonce[3] = {np[0], np[1], np[2]};
  uint32_t ks0[16], rw[4], sw[4];
  cp_block(key, j, nonce, ks0);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    rw[k] = __shfl(ks0[k], 0, (int)kCpRow);
    sw[k] = __shfl(ks0[4 + k], 0, (int)kCpRow);
  }
  // block c's 64 bytes of text; c = 0 and c > nb64 touch nothing (t wraps past nc)
  auto xor_block = [&](uint32_t c, const uint32_t (&ks)[16], uint32_t keep) {
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
      const uint32_t t = 4u * (c - 1u) + q;
      if (t < nc) {
        const uint4 d = SEAL ? *reinterpret_cast<const uint4*>(inp + 16u * t) : X[na + t];
        const uint4 o = ae_keep(make_uint4(d.x ^ ks[4 * q], d.y ^ ks[4 * q + 1], d.z ^ ks[4 * q + 2], d.w ^ ks[4 * q + 3]),
                                (int)text_len - 16 * (int)t);
        if (SEAL) X[na + t] = o;
        *reinterpret_cast<uint4*>(outp + 16u * t) = make_uint4(o.x & keep, o.y & keep, o.z & keep, o.w & keep);
      }
    }
  };
  auto xor_text = [&](uint32_t keep) {
    xor_block(j, ks0, keep);
    for (uint32_t c0 = kCpRow; c0 <= nb64; c0 += kCpRow) {
      uint32_t ks[16];
      cp_block(key, c0 + j, nonce, ks);
      xor_block(c0 + j, ks, keep);
    }
  };
  bool emit = len_ok;
  if (SEAL) {
    if (merge) emit = emit & (a.opened[i] != 0);
    xor_text(emit ? ~0u : 0u);
  }
  wave_lds_sync();

  // 3. the powers of r
  P130 pw = p130_clamp_r(rw);
#pragma unroll
  for (uint32_t s = 1; s < kCpRow; s <<= 1) {
    const P130 pr = p130_mul(cp_row_get(pw, s - 1u), cp_row_get(pw, (j - s) & (s - 1u)));
    const bool take = (j >= s) & (j < 2u * s);
#pragma unroll
    for (int k = 0; k < 5; ++k) pw.v[k] = take ? pr.v[k] : pw.v[k];
  }
  const P130 R = cp_row_get(pw, kCpRow - 1u);

  // 4. Poly1305
  auto block_e = [&](uint32_t e) {  // block e from the end, zero past the first
    const bool has = e < m;
    const uint4 d = X[has ? m - 1u - e : 0u];
    P130 b = p130_of_block(d.x, d.y, d.z, d.w, 1u);
#pragma unroll
    for (int k = 0; k < 5; ++k) b.v[k] = has ? b.v[k] : 0u;
    return b;
  };
  const uint32_t kk = (m + kCpRow - 1u) / kCpRow;  // >= 1
  P130 acc = block_e(j + kCpRow * (kk - 1u));
  for (uint32_t k = kk - 1u; k-- > 0;) acc = p130_add(p130_mul(acc, R), block_e(j + kCpRow * k));
  acc = p130_mul(acc, pw);
#pragma unroll
  for (int off = 1; off < (int)kCpRow; off <<= 1) {
#pragma unroll
    for (int k = 0; k < 5; ++k) acc.v[k] += __shfl_xor(acc.v[k], off, (int)kCpRow);
  }
  uint32_t tg[4];
  p130_finish(acc, sw, tg);
  const uint32_t tq = j >> 2;
  const uint32_t tword = tq == 0 ? tg[0] : tq == 1 ? tg[1] : tq == 2 ? tg[2] : tg[3];
  const uint32_t tbyte = (tword >> (8u * (j & 3u))) & 0xffu;  // tag byte j

  // 5. the verdict and the output slot
  if (!SEAL) {
    uint32_t diff = (uint32_t)inp[text_len + j] ^ tbyte;  // in_stride >= 16 whatever the length
#pragma unroll
    for (int off = 1; off < (int)kCpRow; off <<= 1) diff |= __shfl_xor(diff, off, (int)kCpRow);
    emit = emit & (diff == 0);
    xor_text(emit ? ~0u : 0u);
  }
  for (uint32_t b = nc + j; b < a.out_stride / 16u; b += kCpRow)
    *reinterpret_cast<uint4*>(outp + 16u * b) = make_uint4(0u, 0u, 0u, 0u);
  if (SEAL) {
    // the tag follows the text at any byte offset: byte stores, after the
    // block stores they overlap
    __threadfence_block();
    outp[text_len + j] = (uint8_t)(emit ? tbyte : 0u);
  }
  if (j == 0) {
    a.out_lens[i] = emit ? text_len + (SEAL ? kAeadTag : 0u) : 0u;
    if (a.ok) a.ok[i] = emit ? 1u : 0u;
    if (merge) {
      const uint32_t st = a.status[i];
      a.status[i] = a.opened[i] != 0 ? st : a.bad_status;
    }
  }
}

#endif  // __HIPCC__

}  // namespace gvs
