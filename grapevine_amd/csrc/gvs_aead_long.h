// gvs_aead_long.h — the channel cipher for Noise-size messages: AES-256-GCM
// over texts of up to 65 519 bytes (ciphertext + tag <= 65 535, a Noise
// message), one 256-thread workgroup per message.
//
// k_aead (gvs_aead.h) parks a message's whole hash input in its wave's LDS
// cells, which is where its 2 048-byte ceiling comes from, and folds every 64
// blocks with a shuffle butterfly.  Here nothing of the text is staged and
// GHASH is a strided Horner indexed from the end of the hash input:
//   the hash input is m = na + nc + 1 blocks (AAD, ciphertext, lengths); the
//   block at distance d from the end (the length block is d = 0) belongs to
//   slot d mod kAlT, and thread t owns the slots t and t + 256 (kAlT = 512:
//   the two blocks that one aes256_encrypt2 call serves are two independent
//   chains, so their multiplies interleave).  A slot walks its distances
//   downwards with Y <- Y * H^kAlT ^ X_d, and
//       S = xor over slots s of Y_s * H^(s + 1).
//   Indexed from the end, the ragged tile is the first one and its missing
//   blocks are leading zeros, which Horner ignores: there is no tail case.
// In the streaming loop a block costs one gf128_mul, no LDS traffic and no
// cross-lane move; the powers H^1 .. H^min(m, 512) are made once by log-step
// doubling across the workgroup, and the slot products are folded once per
// message (a wave butterfly, then four cells).
//
// Seal is one pass: a thread loads its plaintext block, XORs the keystream,
// stores the ciphertext block to the output slot and absorbs it.  Open is two
// passes: the ciphertext is hashed and every wave forms the verdict, then the
// ciphertext is read again (from L2), decrypted and stored as text & verdict,
// so a message that fails issues the stores of one that passes.
//
// The schedule (distance map, power table, Horner walk, final products, tag
// and masked output) is host/device code: tests/aead_long_host.cpp steps 256
// thread states through it on the CPU; k_aead_long<SEAL> is its wave form.
//
// What depends on data: as in k_aead, trip counts and addresses follow the
// clear lengths alone; keys, IVs, text and the verdict reach selects only
// (and the AES table's indices, one replica per bank).
#pragma once
#include "gvs_aead.h"

namespace gvs {

constexpr uint32_t kAeadLongTextMax = 65519;    // GVS_AEAD_LONG_TEXT_MAX
constexpr uint32_t kAeadLongStrideMax = 65536;  // text max + tag, rounded up to blocks
constexpr uint32_t kAlThreads = 256;            // threads per message
constexpr uint32_t kAlT = 2 * kAlThreads;       // slots: the Horner stride

// Cells of the workgroup (device: the holes of the AES table's window)
constexpr uint32_t kAlRk = 0;     // 15 round keys
constexpr uint32_t kAlEj = 15;    // E_K(IV | 1)
constexpr uint32_t kAlHp = 16;    // H^1 .. H^512
constexpr uint32_t kAlFold = kAlHp + kAlT;  // one partial sum per wave
constexpr uint32_t kAlCells = kAlFold + kAlThreads / 64;
static_assert(kAlCells * 16 <= 256 * 128, "the window's holes");

// ------------------------------------------------------------------ the schedule

struct AlShape {
  uint32_t text_len, aad_len;
  uint32_t na, nc, m;  // AAD blocks, text blocks, hash blocks
  uint32_t ntile;      // Horner steps of a slot: ceil(m / kAlT)
  uint32_t maxp;       // powers of H in the table: min(m, kAlT)
};

GVS_AE_FN AlShape al_shape(uint32_t text_len, uint32_t aad_len) {
  AlShape s;
  s.text_len = text_len, s.aad_len = aad_len;
  s.na = (aad_len + 15u) / 16u, s.nc = (text_len + 15u) / 16u;
  s.m = s.na + s.nc + 1u;
  s.ntile = (s.m + kAlT - 1u) / kAlT;
  s.maxp = s.m < kAlT ? s.m : kAlT;
  return s;
}

GVS_AE_FN uint4 al_ld(const uint8_t* p) { return *reinterpret_cast<const uint4*>(p); }
GVS_AE_FN void al_st(uint8_t* p, uint4 v) { *reinterpret_cast<uint4*>(p) = v; }
GVS_AE_FN Gf128 al_gf(uint4 d) { return Gf128{{d.x, d.y, d.z, d.w}}; }
GVS_AE_FN uint4 al_u4(const Gf128& g) { return make_uint4(g.w[0], g.w[1], g.w[2], g.w[3]); }

// the first nbytes bytes of a block of little-endian memory words
GVS_AE_FN uint4 al_keep(uint4 v, int nbytes) {
#if defined(__HIP_DEVICE_COMPILE__)
  return ae_keep(v, nbytes);
#else
  uint32_t w[4] = {v.x, v.y, v.z, v.w};
  for (int k = 0; k < 16; ++k)
    if (k >= nbytes) w[k >> 2] &= ~(0xffu << (8 * (k & 3)));
  return make_uint4(w[0], w[1], w[2], w[3]);
#endif
}

// keystream block (big-endian words) over a block of memory words
GVS_AE_FN uint4 al_xor_ks(uint4 d, const uint32_t (&ks)[4]) {
  return make_uint4(d.x ^ bswap32(ks[0]), d.y ^ bswap32(ks[1]), d.z ^ bswap32(ks[2]), d.w ^ bswap32(ks[3]));
}

// Doubling step `step` (1, 2, 4 .. 256) of the power table, thread t: cells
// [step, 2 step) = H^step * cells [0, step).  A step reads below `step` and
// writes at or above it, so one barrier between steps is enough.  hp[i] = H^(i+1).
template <typename Cells>
GVS_AE_FN void al_pow_step(Cells&& hp, uint32_t step, uint32_t t) {
  const Gf128 pr = gf128_mul(al_gf(hp[step - 1u]), al_gf(hp[t & (step - 1u)]));
  if (t < step) hp[step + t] = al_u4(pr);
}

// Tile k of thread t: the Horner step of its two slots, at the distances
// kAlT k + t + 256 and kAlT k + t from the end of the hash input.  A text
// block is read from `in`; a sealing thread encrypts it (counter = text block
// + 2), stores it to `out` and absorbs the ciphertext.  `first`: the slot
// values are still zero, so the multiply is skipped (the tile with k = ntile - 1).
// ht: H^512.  Block reads stay inside the slots: in_stride and aad_stride are
// multiples of 16 that hold the lengths.
template <bool SEAL, typename Rk, typename Tab>
GVS_AE_FN void al_tile(const AlShape& s, const Rk& rk, const Tab& te, const uint32_t (&iv)[3],
                       const uint8_t* aad, const uint8_t* in, uint8_t* out, uint32_t k, uint32_t t,
                       bool first, const Gf128& ht, Gf128 (&y)[2]) {
  uint32_t d[2], g[2], c[2];
  bool text[2], is_aad[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    d[j] = kAlT * k + (j ? 0u : kAlThreads) + t;
    g[j] = s.m - 1u - d[j];  // the block's place from the front; wraps past the front
    c[j] = g[j] - s.na;      // its text block
    const bool live = d[j] < s.m;
    is_aad[j] = live & (g[j] < s.na);
    text[j] = live & (g[j] >= s.na) & (d[j] != 0u);
  }
  uint32_t ka[4] = {iv[0], iv[1], iv[2], c[0] + 2u}, kb[4] = {iv[0], iv[1], iv[2], c[1] + 2u};
  if (SEAL) aes256_encrypt2(rk, te, ka, kb);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    uint4 x = make_uint4(0u, 0u, 0u, 0u);
    if (text[j]) {
      const uint4 v = al_ld(in + 16u * c[j]);
      const int nb = (int)s.text_len - 16 * (int)c[j];
      if (SEAL) {
        x = al_keep(al_xor_ks(v, j ? kb : ka), nb);
        al_st(out + 16u * c[j], x);
      } else {
        x = al_keep(v, nb);
      }
    }
    if (is_aad[j]) x = al_keep(al_ld(aad + 16u * g[j]), (int)s.aad_len - 16 * (int)g[j]);
    if (d[j] == 0u) x = make_uint4(0u, bswap32(s.aad_len * 8u), 0u, bswap32(s.text_len * 8u));
    const Gf128 xb = gf128_of_block(x);
    const int q = 1 - j;  // y[0]: slot t, y[1]: slot t + 256
    if (!first) y[q] = gf128_mul(y[q], ht);
#pragma unroll
    for (int w = 0; w < 4; ++w) y[q].w[w] ^= xb.w[w];
  }
}

// thread t's share of S: its slots' values times H^(slot + 1).  A slot at or
// past m has absorbed nothing; its product is zero whatever power it reads,
// and a wave (first thread wbase) whose 64 slots are all past m skips the
// multiply: a uniform branch on the clear lengths.
template <typename Cells>
GVS_AE_FN Gf128 al_final(const AlShape& s, Cells&& hp, uint32_t t, uint32_t wbase, const Gf128 (&y)[2]) {
  Gf128 p{{0, 0, 0, 0}};
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    if (wbase + (uint32_t)q * kAlThreads >= s.m) continue;
    const uint32_t slot = t + (uint32_t)q * kAlThreads;
    const Gf128 pr = gf128_mul(y[q], al_gf(hp[slot < s.maxp ? slot : 0u]));
#pragma unroll
    for (int w = 0; w < 4; ++w) p.w[w] ^= pr.w[w];
  }
  return p;
}

// byte i of the tag S ^ E_K(IV | 1) (ej as big-endian words)
GVS_AE_FN uint32_t al_tag_byte(const Gf128& sum, const uint4& ej, uint32_t i) {
  const uint32_t q = (i >> 2) & 3u;
  const uint32_t w = q == 0 ? sum.w[3] ^ ej.x : q == 1 ? sum.w[2] ^ ej.y : q == 2 ? sum.w[1] ^ ej.z : sum.w[0] ^ ej.w;
  return (w >> (24u - 8u * (i & 3u))) & 0xffu;
}

// The open path's second pass, tile k of thread t: text blocks kAlT k + t and
// + 256 are read again, decrypted and stored under the verdict's mask
// (`keep`: all ones or zero), the same stores either way.
template <typename Rk, typename Tab>
GVS_AE_FN void al_open_tile(const AlShape& s, const Rk& rk, const Tab& te, const uint32_t (&iv)[3],
                            const uint8_t* in, uint8_t* out, uint32_t k, uint32_t t, uint32_t keep) {
  const uint32_t c[2] = {kAlT * k + t, kAlT * k + t + kAlThreads};
  uint32_t ka[4] = {iv[0], iv[1], iv[2], c[0] + 2u}, kb[4] = {iv[0], iv[1], iv[2], c[1] + 2u};
  aes256_encrypt2(rk, te, ka, kb);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (c[j] < s.nc) {
      const uint4 o = al_keep(al_xor_ks(al_ld(in + 16u * c[j]), j ? kb : ka), (int)s.text_len - 16 * (int)c[j]);
      al_st(out + 16u * c[j], make_uint4(o.x & keep, o.y & keep, o.z & keep, o.w & keep));
    }
  }
}

// ------------------------------------------------------------------ the kernel

#if defined(__HIPCC__)

struct AlCells {
  uint32_t* s_te;
  uint32_t base;
  __device__ uint4& operator[](uint32_t i) const { return *ae_cell(s_te, base + i); }
};

// One workgroup per message (grid = n); AeadArgs without the wire call's merge.
//  1. wave 0 expands the key into cells and computes H = E_K(0) and
//     E_K(IV | 1); round-key reads are broadcasts from then on
//  2. the power table, log2(min(m, 512)) doubling steps; a step below 256
//     occupies its first step / 64 waves only
//  3. the tiles, from the ragged one at the front down to the one that ends
//     with the length block (seal: ciphertext blocks go out as they are made)
//  4. the slot products, XOR-folded by a wave butterfly and four cells
//  5. open: every wave compares the tag (lanes 0..15 a byte each, a ballot),
//     then the second pass; both: zeros from the text's end to the stride,
//     seal's tag bytes after the block stores they overlap
template <bool SEAL>
__global__ void __launch_bounds__(kAlThreads) k_aead_long(AeadArgs a) {
  GVS_TE_LDS s_te[kTeWords];
  load_te(s_te, a.te);
  __syncthreads();
  const uint32_t t = threadIdx.x, lane = lane_id();
  const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const uint32_t i = blockIdx.x;
  const LdsTe te = lds_te(s_te);

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
  const AlShape s = al_shape(len_ok ? text_len : 0u, len_ok ? aad_len : 0u);

  const AeRk rk{s_te, kAlRk};
  const AlCells hp{s_te, kAlHp}, cells{s_te, 0u};
  const uint32_t* ivp = a.ivs + 3 * (uint64_t)i;
  const uint32_t iv[3] = {bswap32(ivp[0]), bswap32(ivp[1]), bswap32(ivp[2])};
  const uint8_t* aadp = a.aad + (uint64_t)i * a.aad_stride;
  const uint8_t* inp = a.in + (uint64_t)i * a.in_stride;
  uint8_t* outp = a.out + (uint64_t)i * a.out_stride;

  // 1. the key schedule, the hash key and the tag's mask
  if (wave == 0) {
    const uint4 k0 = a.keys[2 * (uint64_t)i], k1 = a.keys[2 * (uint64_t)i + 1];
    const uint32_t kw[8] = {bswap32(k0.x), bswap32(k0.y), bswap32(k0.z), bswap32(k0.w),
                            bswap32(k1.x), bswap32(k1.y), bswap32(k1.z), bswap32(k1.w)};
    uint32_t w[60];
    aes256_expand(te, kw, w);
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < 15; ++r) cells[kAlRk + r] = make_uint4(w[4 * r], w[4 * r + 1], w[4 * r + 2], w[4 * r + 3]);
    }
    wave_lds_sync();
    uint32_t hb[4] = {0, 0, 0, 0}, ej[4] = {iv[0], iv[1], iv[2], 1u};
    aes256_encrypt2(rk, te, hb, ej);
    if (lane == 0) {
      hp[0] = make_uint4(hb[3], hb[2], hb[1], hb[0]);
      cells[kAlEj] = make_uint4(ej[0], ej[1], ej[2], ej[3]);
    }
  }
  __syncthreads();

  // 2. the powers of H
  for (uint32_t step = 1; step < s.maxp; step <<= 1) {
    if (wave * 64u < step) al_pow_step(hp, step, t);  // a wave past the step's threads has nothing to store
    __syncthreads();
  }
  const uint4 htc = hp[s.m > kAlT ? kAlT - 1u : 0u];  // read by tiles after the first only
  const Gf128 ht = al_gf(htc);

  // 3. the tiles
  Gf128 y[2] = {{{0, 0, 0, 0}}, {{0, 0, 0, 0}}};
  for (uint32_t k = s.ntile; k-- > 0;) al_tile<SEAL>(s, rk, te, iv, aadp, inp, outp, k, t, k + 1u == s.ntile, ht, y);

  // 4. S
  Gf128 p = al_final(s, hp, t, wave * 64u, y);
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
    for (int w = 0; w < 4; ++w) p.w[w] ^= __shfl_xor(p.w[w], off);
  }
  if (lane == 0) cells[kAlFold + wave] = al_u4(p);
  __syncthreads();
  Gf128 sum{{0, 0, 0, 0}};
#pragma unroll
  for (uint32_t v = 0; v < kAlThreads / 64; ++v) {
    const uint4 f = cells[kAlFold + v];
    sum.w[0] ^= f.x, sum.w[1] ^= f.y, sum.w[2] ^= f.z, sum.w[3] ^= f.w;
  }
  const uint4 ej = cells[kAlEj];
  const uint32_t tbyte = al_tag_byte(sum, ej, lane & 15u);

  // 5. the verdict and the output slot
  bool emit = len_ok;
  if (!SEAL) {
    const uint32_t theirs = inp[s.text_len + (lane & 15u)];  // in_stride >= 16 whatever the length
    const bool differs = (lane < 16u) & (theirs != tbyte);
    emit = emit & (__ballot(differs) == 0);
    const uint32_t keep = emit ? ~0u : 0u;
    for (uint32_t k = 0; k < (s.nc + kAlT - 1u) / kAlT; ++k) al_open_tile(s, rk, te, iv, inp, outp, k, t, keep);
  }
  for (uint32_t b = s.nc + t; b < a.out_stride / 16u; b += kAlThreads)
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
