// gvs_chachapoly_long.h — ChaCha20-Poly1305 for Noise-size messages: texts of
// up to 65 519 bytes (ciphertext + tag <= 65 535, a Noise message), one
// 256-thread workgroup per message.  The limits are those of
// k_aead_long (gvs_aead_long.h); the primitives are those of gvs_chachapoly.h.
//
// k_chachapoly parks a message's MAC input in its row's LDS cells, which is
// where its 2 048-byte ceiling comes from.  Here nothing of the text is staged.
//
// The chunk grid.  The MAC input pad16(AAD) | pad16(C) | lengths is laid on a
// grid of 64-byte chunks of four 16-byte cells:
//   cell 4 + c        text block c                  (c < nc)
//   cell 4 - na + g   AAD block g                   (g < na <= 4)
//   cell 4 + nc       the length block
// so the grid starts at cell 4 - na and ends at cell E = nc + 5 whatever the
// AAD length is, and chunk Q is exactly ChaCha20 block counter Q: chunk 0 is
// the one-time-key block (it carries the AAD and is XORed over nothing), chunk
// Q >= 1 is the keystream of text bytes [64 (Q - 1), 64 Q).  Thread t owns the
// chunks Q = t (mod 256); a tile is 256 chunks (16 KiB), and the largest
// message is four tiles and a fifth with thread 0 alone.
//
// Poly1305 is a 1 024-way strided Horner from the front: thread t keeps four
// accumulators, one per cell column u of its chunks, and per tile
//   y_u <- y_u * R + X,   R = r^1024:
// four independent chains per thread, no LDS traffic and no cross-lane move in
// the loop.  A cell before the grid's start adds nothing (y stays zero); a cell
// at or past E is neither added nor multiplied (a select on the clear
// lengths).  After the tiles accumulator (t, u) is multiplied once by
// r^(E - p_last), p_last its last live cell, an exponent in 1 .. 1 024 that
// follows the clear lengths only.  The powers r^1 .. r^min(E, 1024) are made
// once per message by log-step doubling across the workgroup into LDS, five
// limbs an entry (20 KiB), one barrier a step.  The 1 024 products are summed
// limb by limb (see cl_final and the kernel's fold for the bounds).
//
// Seal is one pass: a thread makes its chunk's keystream block in registers,
// loads 64 bytes of text, XORs, stores the ciphertext and absorbs it.  Open is
// two passes: the received ciphertext is hashed and every wave forms the
// verdict, then the ciphertext is read again (from L2), XORed and stored as
// text & verdict, so a message that fails issues the stores of one that passes.
//
// The schedule (cell map, power steps, tile step, final exponents, masked
// second pass) is host/device code: tests/chachapoly_long_host.cpp steps 256
// thread states through it on the CPU; k_chachapoly_long<SEAL> is its wave form.
//
// What depends on data: trip counts, addresses and table indices follow the
// clear lengths alone; keys, nonces, text, r, s, the powers and the verdict
// reach selects only.  No table of the cipher, no scratch.
#pragma once
#include "gvs_aead_long.h"
#include "gvs_chachapoly.h"

namespace gvs {

constexpr uint32_t kClThreads = 256;        // threads per message
constexpr uint32_t kClT = 4 * kClThreads;   // cells per tile: the Horner stride
// Words of the workgroup
constexpr uint32_t kClPw = 0;               // limb k of r^(i + 1) at kClPw + kClT k + i
constexpr uint32_t kClS = kClPw + 5 * kClT; // s, four words
constexpr uint32_t kClFold = kClS + 4;      // one partial sum per wave: five limbs in eight words
constexpr uint32_t kClWords = kClFold + 8 * (kClThreads / 64);

// ------------------------------------------------------------------ the schedule

struct ClShape {
  uint32_t text_len, aad_len;
  uint32_t na, nc;
  uint32_t start, end;  // the grid's first live cell and the cell after its last (E)
  uint32_t ntile;       // tiles: ceil(E / kClT)
  uint32_t maxp;        // powers of r in the table: min(E, kClT)
};

// a grid of the cells [start, end)
GVS_CP_FN ClShape cl_grid(uint32_t start, uint32_t end) {
  ClShape s{};
  s.start = start, s.end = end;
  s.ntile = (end + kClT - 1u) / kClT;
  s.maxp = end < kClT ? end : kClT;
  return s;
}

GVS_CP_FN ClShape cl_shape(uint32_t text_len, uint32_t aad_len) {
  const uint32_t na = (aad_len + 15u) / 16u, nc = (text_len + 15u) / 16u;
  ClShape s = cl_grid(4u - na, nc + 5u);
  s.text_len = text_len, s.aad_len = aad_len, s.na = na, s.nc = nc;
  return s;
}

GVS_CP_FN P130 cl_pw_get(const uint32_t* w, uint32_t i) {
  return P130{{w[kClPw + i], w[kClPw + kClT + i], w[kClPw + 2u * kClT + i], w[kClPw + 3u * kClT + i],
               w[kClPw + 4u * kClT + i]}};
}

GVS_CP_FN void cl_pw_put(uint32_t* w, uint32_t i, const P130& p) {
#pragma unroll
  for (uint32_t k = 0; k < 5; ++k) w[kClPw + kClT * k + i] = p.v[k];
}

// Doubling step `step` (1, 2, 4 .. 512) of the power table, thread t: entries
// [step, 2 step) = r^step * entries [0, step), cut at maxp; entry i is
// r^(i + 1).  Steps 256 and 512 give a thread one and two entries.  A step
// reads below `step` and writes at or above it, so one barrier between steps is
// enough.  Both factors are carried (entry 0 is the clamped r, below 2^26 a
// limb; the others are products of p130_mul).
GVS_CP_FN void cl_pow_step(uint32_t* w, uint32_t step, uint32_t maxp, uint32_t t) {
  const P130 top = cl_pw_get(w, step - 1u);
  for (uint32_t i = t; i < step && step + i < maxp; i += kClThreads)
    cl_pw_put(w, step + i, p130_mul(top, cl_pw_get(w, i)));
}

// One Horner step of the accumulator that owns cell p, x the cell's 16 bytes.
// `first`: tile 0, where the accumulator is still zero and the multiply is
// skipped.  Limbs: R carried; y enters below 2^27 + 2^10 (p130_mul's bound for
// its left factor) and leaves as a carried product (below 2^26 + 2^9) plus a
// block with its 2^128 bit (below 2^26): below 2^27 + 2^9.
GVS_CP_FN void cl_absorb(const ClShape& s, uint32_t p, uint4 x, bool first, const P130& R, P130& y) {
  const bool live = (p >= s.start) & (p < s.end);
  const P130 b = p130_of_block(x.x, x.y, x.z, x.w, 1u);
  P130 m{{0, 0, 0, 0, 0}};
  if (!first) m = p130_mul(y, R);
#pragma unroll
  for (int k = 0; k < 5; ++k) y.v[k] = live ? m.v[k] + b.v[k] : y.v[k];
}

GVS_CP_FN uint4 cl_xor_ks(uint4 d, const uint32_t (&ks)[16], uint32_t u) {
  return make_uint4(d.x ^ ks[4u * u], d.y ^ ks[4u * u + 1u], d.z ^ ks[4u * u + 2u], d.w ^ ks[4u * u + 3u]);
}

// Chunk Q of its thread: the four cells 4 Q + u.  A text block is read from
// `in`; a sealing thread XORs ks (ChaCha20 block Q; not read otherwise) over
// it, stores it to `out` and absorbs the ciphertext.  Block reads stay inside
// the slots: in_stride and aad_stride are multiples of 16 that hold the lengths.
template <bool SEAL>
GVS_CP_FN void cl_tile(const ClShape& s, const uint32_t (&ks)[16], const uint8_t* aad, const uint8_t* in,
                       uint8_t* out, uint32_t Q, bool first, const P130& R, P130 (&y)[4]) {
#pragma unroll
  for (uint32_t u = 0; u < 4; ++u) {
    const uint32_t p = 4u * Q + u, c = p - 4u, g = p - s.start;  // c wraps in chunk 0, g before the grid
    uint4 x = make_uint4(0u, 0u, 0u, 0u);
    if ((p >= 4u) & (c < s.nc)) {
      const uint4 v = al_ld(in + 16u * c);
      const int nb = (int)s.text_len - 16 * (int)c;
      if (SEAL) {
        x = al_keep(cl_xor_ks(v, ks, u), nb);
        al_st(out + 16u * c, x);
      } else {
        x = al_keep(v, nb);
      }
    }
    if ((p < 4u) & (p >= s.start)) x = al_keep(al_ld(aad + 16u * g), (int)s.aad_len - 16 * (int)g);
    if (p == 4u + s.nc) x = make_uint4(s.aad_len, 0u, s.text_len, 0u);
    cl_absorb(s, p, x, first, R, y[u]);
  }
}

// Thread t's share of the MAC: accumulator u (cells 4 t + u mod 1 024) times
// r^(E - p_last).  With slot = 4 t + u < E, E - p_last = ((E - 1 - slot) mod
// 1 024) + 1, which is at most min(E, 1 024): inside the table.  A slot at or
// past E has absorbed nothing and its product is zero whatever power it reads;
// a wave (first thread wbase) whose slots are all past E skips the multiplies,
// a uniform branch on the clear lengths.  The four products are carried, so a
// limb of their sum is below 2^28 + 2^11; one carry pass inside brings every
// limb back to 2^26 or below before the fold.
GVS_CP_FN P130 cl_final(const ClShape& s, const uint32_t* w, uint32_t t, uint32_t wbase, const P130 (&y)[4]) {
  P130 sum{{0, 0, 0, 0, 0}};
  if (4u * wbase >= s.end) return sum;
#pragma unroll
  for (uint32_t u = 0; u < 4; ++u) {
    const uint32_t slot = 4u * t + u;
    const uint32_t e = slot < s.end ? (s.end - 1u - slot) & (kClT - 1u) : 0u;
    sum = p130_add(sum, p130_mul(y[u], cl_pw_get(w, e)));
  }
  p130_carry(sum);
  return sum;
}

GVS_CP_FN uint32_t cl_tag_byte(const uint32_t (&tg)[4], uint32_t i) {
  const uint32_t q = (i >> 2) & 3u;
  const uint32_t w = q == 0 ? tg[0] : q == 1 ? tg[1] : q == 2 ? tg[2] : tg[3];
  return (w >> (8u * (i & 3u))) & 0xffu;
}

// The open path's second pass, chunk Q of its thread: its text blocks are read
// again, XORed with ks (ChaCha20 block Q) and stored under the verdict's mask
// (`keep`: all ones or zero), the same stores either way.
GVS_CP_FN void cl_open_tile(const ClShape& s, const uint32_t (&ks)[16], const uint8_t* in, uint8_t* out,
                            uint32_t Q, uint32_t keep) {
#pragma unroll
  for (uint32_t u = 0; u < 4; ++u) {
    const uint32_t c = 4u * (Q - 1u) + u;  // wraps in chunk 0
    if ((Q >= 1u) & (c < s.nc)) {
      const uint4 o = al_keep(cl_xor_ks(al_ld(in + 16u * c), ks, u), (int)s.text_len - 16 * (int)c);
      al_st(out + 16u * c, make_uint4(o.x & keep, o.y & keep, o.z & keep, o.w & keep));
    }
  }
}

// ------------------------------------------------------------------ the kernel

#if defined(__HIPCC__)

__device__ inline P130 cl_uniform(const P130& p) {
  P130 o;
#pragma unroll
  for (int k = 0; k < 5; ++k) o.v[k] = __builtin_amdgcn_readfirstlane(p.v[k]);
  return o;
}

// Open's tile-0 keystream block: kept in registers across the hash pass and
// the verdict (true), or made again in the second pass (false).  DESIGN.md §20
// has the register counts and the measured run that decided it.
#ifndef GVS_CL_OPEN_KEEPS_BLOCK0
#define GVS_CL_OPEN_KEEPS_BLOCK0 0
#endif

// One workgroup per message (grid = n); AeadArgs without `te` and without the
// wire call's merge.
//  1. every thread makes ChaCha20 block t, tile 0's (an opening workgroup that
//     makes it again in its second pass: wave 0 only); thread 0's is the
//     one-time key: r (clamped) becomes entry 0 of the power table and s goes
//     to four words beside it
//  2. the power table, log2(min(E, 1024)) doubling steps; a step below 256
//     occupies its first step / 64 waves only
//  3. the tiles from the front (seal: ciphertext blocks go out as they are
//     made); a wave whose chunks all lie past E skips the tile
//  4. the final products, summed limb by limb: a wave butterfly with one carry
//     pass in the middle, then four cells; p130_finish adds s
//  5. open: every wave compares the tag (lanes 0..15 a byte each, a ballot),
//     then the second pass; both: zeros from the text's end to the stride,
//     seal's tag bytes after the block stores they overlap
template <bool SEAL>
__global__ void __launch_bounds__(kClThreads) k_chachapoly_long(AeadArgs a) {
  __shared__ uint32_t s_w[kClWords];
  constexpr bool kHold = SEAL || GVS_CL_OPEN_KEEPS_BLOCK0;  // block t stays in registers for tile 0's text
  const uint32_t t = threadIdx.x, lane = lane_id();
  const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const uint32_t i = blockIdx.x;

  // lengths: uniform, and the only data that loops and addresses follow
  const uint32_t in_len = __builtin_amdgcn_readfirstlane(a.in_lens[i]);
  uint32_t aad_len = a.aad ? __builtin_amdgcn_readfirstlane(a.aad_lens[i]) : 0u;
  bool len_ok = in_len <= a.in_stride && aad_len <= kAeadAadMax && aad_len <= a.aad_stride;
  uint32_t text_len;
  if (SEAL) {
    text_len = in_len;
    len_ok = len_ok & (text_len <= kAeadLongTextMax) & ((uint64_t)text_len + kAeadTag <= a.out_stride);
  } else {
    len_ok = len_ok & (in_len >= kAeadTag);
    text_len = in_len - kAeadTag;
    len_ok = len_ok & (text_len <= kAeadLongTextMax) & (text_len <= a.out_stride);
  }
  const ClShape s = cl_shape(len_ok ? text_len : 0u, len_ok ? aad_len : 0u);

  const uint4 k0 = a.keys[2 * (uint64_t)i], k1 = a.keys[2 * (uint64_t)i + 1];
  const uint32_t key[8] = {k0.x, k0.y, k0.z, k0.w, k1.x, k1.y, k1.z, k1.w};
  const uint32_t* np = a.ivs + 3 * (uint64_t)i;
  const uint32_t nonce[3] = {np[0], np[1], np[2]};
  const uint8_t* aadp = a.aad + (uint64_t)i * a.aad_stride;
  const uint8_t* inp = a.in + (uint64_t)i * a.in_stride;
  uint8_t* outp = a.out + (uint64_t)i * a.out_stride;

  // 1. block t, and the one-time key
  uint32_t ks0[16] = {};
  if (kHold || wave == 0) {
    cp_block(key, t, nonce, ks0);
    if (t == 0) {
      const uint32_t rw[4] = {ks0[0], ks0[1], ks0[2], ks0[3]};
      cl_pw_put(s_w, 0u, p130_clamp_r(rw));
#pragma unroll
      for (int k = 0; k < 4; ++k) s_w[kClS + k] = ks0[4 + k];
    }
  }
  __syncthreads();

  // 2. the powers of r
  for (uint32_t step = 1; step < s.maxp; step <<= 1) {
    if (wave * 64u < step) cl_pow_step(s_w, step, s.maxp, t);  // a wave past the step's threads has nothing to store
    __syncthreads();
  }
  const P130 R = cl_uniform(cl_pw_get(s_w, s.end > kClT ? kClT - 1u : 0u));  // read by tiles after the first only

  // 3. the tiles
  P130 y[4] = {{{0, 0, 0, 0, 0}}, {{0, 0, 0, 0, 0}}, {{0, 0, 0, 0, 0}}, {{0, 0, 0, 0, 0}}};
  if (4u * 64u * wave < s.end) cl_tile<SEAL>(s, ks0, aadp, inp, outp, t, true, R, y);
  for (uint32_t k = 1; k < s.ntile; ++k) {
    if (4u * (kClThreads * k + 64u * wave) >= s.end) continue;  // the ragged last tile, by waves
    const uint32_t Q = kClThreads * k + t;
    if (SEAL) {
      uint32_t ks[16];
      cp_block(key, Q, nonce, ks);
      cl_tile<true>(s, ks, aadp, inp, outp, Q, false, R, y);
    } else {
      cl_tile<false>(s, ks0, aadp, inp, outp, Q, false, R, y);
    }
  }

  // 4. the MAC.  A thread's sum comes carried (limbs at most 2^26): 16 of them
  // stay at or below 2^30; a carry pass; the other four lanes' give at most
  // 2^28, and the four waves' 2^30, inside p130_finish's 2^31.
  P130 p = cl_final(s, s_w, t, 64u * wave, y);
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) {
#pragma unroll
    for (int k = 0; k < 5; ++k) p.v[k] += __shfl_xor(p.v[k], off);
  }
  p130_carry(p);
#pragma unroll
  for (int off = 16; off < 64; off <<= 1) {
#pragma unroll
    for (int k = 0; k < 5; ++k) p.v[k] += __shfl_xor(p.v[k], off);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 5; ++k) s_w[kClFold + 8u * wave + k] = p.v[k];
  }
  __syncthreads();
  P130 h{{0, 0, 0, 0, 0}};
#pragma unroll
  for (uint32_t v = 0; v < kClThreads / 64; ++v) {
#pragma unroll
    for (int k = 0; k < 5; ++k) h.v[k] += s_w[kClFold + 8u * v + k];
  }
  const uint32_t sw[4] = {s_w[kClS], s_w[kClS + 1], s_w[kClS + 2], s_w[kClS + 3]};
  uint32_t tg[4];
  p130_finish(h, sw, tg);
  const uint32_t tbyte = cl_tag_byte(tg, lane & 15u);

  // 5. the verdict and the output slot
  bool emit = len_ok;
  if (!SEAL) {
    const uint32_t theirs = inp[s.text_len + (lane & 15u)];  // in_stride >= 16 whatever the length
    const bool differs = (lane < 16u) & (theirs != tbyte);
    emit = emit & (__ballot(differs) == 0);
    const uint32_t keep = emit ? ~0u : 0u;
    const uint32_t nchunk = s.nc ? (s.nc + 3u) / 4u + 1u : 0u;  // chunk 0 and the text's
    for (uint32_t k = 0; kClThreads * k + 64u * wave < nchunk; ++k) {
      const uint32_t Q = kClThreads * k + t;
      if (k == 0 && kHold) {
        cl_open_tile(s, ks0, inp, outp, Q, keep);
      } else {
        uint32_t ks[16];
        cp_block(key, Q, nonce, ks);
        cl_open_tile(s, ks, inp, outp, Q, keep);
      }
    }
  }
  for (uint32_t b = s.nc + t; b < a.out_stride / 16u; b += kClThreads)
    al_st(outp + 16u * b, make_uint4(0u, 0u, 0u, 0u));
  if (SEAL) {
    // the tag follows the text at any byte offset: byte stores, after the
    // block stores (of other waves too) that they overlap
    __syncthreads();
    if (t < 16u) outp[s.text_len + t] = (uint8_t)(emit ? tbyte : 0u);
  }
  if (t == 0) {
    a.out_lens[i] = emit ? s.text_len + (SEAL ? kAeadTag : 0u) : 0u;
    if (a.ok) a.ok[i] = emit ? 1u : 0u;
  }
}

#endif  // __HIPCC__

}  // namespace gvs
