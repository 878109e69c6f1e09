// gvs_aead.h — the attested channel's cipher on the device: AES-256-GCM (NIST
// SP 800-38D, 96-bit IV, 128-bit tag), batched over messages that each have a
// key of their own.
//
// The reference wraps every QueryRequest / QueryResponse in an mc-noise
// ciphertext (README.md:177-185 of the reference); Noise's AESGCM cipher is
// AES-256-GCM with the nonce 0^32 | be64(counter).  Per message:
//   H   = E_K(0^128)                      the hash key
//   ks_j = E_K(IV | be32(j + 2))          keystream block j, C_j = P_j ^ ks_j
//   S   = GHASH_H(AAD pad | C pad | be64(8 |AAD|) | be64(8 |C|))
//   tag = S ^ E_K(IV | be32(1))
//
// The primitives (AES-256 key expansion and block function over the project's
// te0 table, the GF(2^128) multiply, a serial whole-message form) are
// host/device code, so tests/aead_host.cpp runs them on the CPU.  The kernel,
// k_aead<SEAL>, is their wave form.
//
// GF(2^128): gfx950 has no carry-less multiply.  gf128_mul is 32 masked
// shift-and-xor steps of four multiplier bits each (one per word of the
// multiplier) into a 256-bit product, then one reduction; no table, no
// branch, every index a constant (DESIGN.md §14 has the instruction count
// against the integer-multiply "holes" method).
//
// What depends on data: loop trip counts follow a message's length and AAD
// length, which the caller passes in clear.  Keys, IVs, text and the outcome
// of the tag comparison reach no branch and no address, apart from the AES
// table indices (gvs_seal_dev.h: one replica per bank, so no timing through
// conflicts).  A message that fails is zeroed through selects; its stores are
// the stores of one that passes.
#pragma once
#include "gvs_seal_dev.h"

namespace gvs {

#define GVS_AE_FN __host__ __device__ __attribute__((always_inline)) inline

constexpr uint32_t kAeadTextMax = 2048;  // GVS_AEAD_TEXT_MAX
constexpr uint32_t kAeadAadMax = 64;     // GVS_AEAD_AAD_MAX
constexpr uint32_t kAeadTag = 16;
constexpr uint32_t kAeadIv = 12;
constexpr uint32_t kAeadMsgs = 4;        // messages (waves) per workgroup

// ------------------------------------------------------------------ AES-256

// SubWord (FIPS-197 §5.2): the S-box is byte 1 of a te0 entry
template <typename Tab>
GVS_AE_FN uint32_t aes_subword(const Tab& te0, uint32_t t) {
  return ((te_at(te0, t, 3) << 16) & 0xff000000u) | ((te_at(te0, t, 2) << 8) & 0x00ff0000u) |
         (te_at(te0, t, 1) & 0x0000ff00u) | ((te_at(te0, t, 0) >> 8) & 0xffu);
}

// the 60 round-key words (big-endian) of a 256-bit key given as 8 big-endian words
template <typename Tab>
GVS_AE_FN void aes256_expand(const Tab& te0, const uint32_t key[8], uint32_t w[60]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = key[i];
  uint32_t rcon = 0x01000000u;
#pragma unroll
  for (int i = 8; i < 60; ++i) {
    uint32_t t = w[i - 1];
    if (i % 8 == 0) {
      t = aes_subword(te0, ror32(t, 24)) ^ rcon;  // RotWord = rotate left by 8
      rcon <<= 1;                                  // 01 .. 40: no reduction needed
    } else if (i % 8 == 4) {
      t = aes_subword(te0, t);
    }
    w[i] = w[i - 8] ^ t;
  }
}

// S-box bytes of four lookups packed big-endian
GVS_AE_FN uint32_t aes_sb4(uint32_t l0, uint32_t l1, uint32_t l2, uint32_t l3) {
#if defined(__HIP_DEVICE_COMPILE__)
  return sbox_pack(l0, l1, l2, l3);
#else
  return ((l0 << 16) & 0xff000000u) | ((l1 << 8) & 0x00ff0000u) | (l2 & 0x0000ff00u) | ((l3 >> 8) & 0xffu);
#endif
}

// The 14-round block function on two blocks at once (the scheme of
// aes128_rounds2: all 32 lookups of a round issued before they are combined).
// rk[r]: round key r as four big-endian words (an array on the host; on the
// device AeRk, the wave's LDS cells, where every lane reads the same address:
// a broadcast).  a, b: the blocks as big-endian words, in and out.
template <typename Rk, typename Tab>
GVS_AE_FN void aes256_encrypt2(const Rk& rk, const Tab& te, uint32_t (&a)[4], uint32_t (&b)[4]) {
  {
    const uint4 k = rk[0];
    a[0] ^= k.x, a[1] ^= k.y, a[2] ^= k.z, a[3] ^= k.w;
    b[0] ^= k.x, b[1] ^= k.y, b[2] ^= k.z, b[3] ^= k.w;
  }
#pragma unroll
  for (int r = 1; r <= 14; ++r) {
    uint32_t la[16], lb[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        la[4 * i + k] = te_at(te, a[(i + k) & 3], 3 - k);
        lb[4 * i + k] = te_at(te, b[(i + k) & 3], 3 - k);
      }
    }
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_sched_barrier(0);
#endif
    const uint4 k4 = rk[r];
    const uint32_t kw[4] = {k4.x, k4.y, k4.z, k4.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (r < 14) {
        a[i] = xor3(xor3(la[4 * i], ror32(la[4 * i + 1], 8), ror32(la[4 * i + 2], 16)),
                    ror32(la[4 * i + 3], 24), kw[i]);
        b[i] = xor3(xor3(lb[4 * i], ror32(lb[4 * i + 1], 8), ror32(lb[4 * i + 2], 16)),
                    ror32(lb[4 * i + 3], 24), kw[i]);
      } else {  // last round: SubBytes + ShiftRows, AddRoundKey
        a[i] = aes_sb4(la[4 * i], la[4 * i + 1], la[4 * i + 2], la[4 * i + 3]) ^ kw[i];
        b[i] = aes_sb4(lb[4 * i], lb[4 * i + 1], lb[4 * i + 2], lb[4 * i + 3]) ^ kw[i];
      }
    }
  }
}

// ------------------------------------------------------------------ GF(2^128)

// A GCM field element as the 128-bit big-endian integer of its 16 bytes,
// w[0] the least significant word: w[3] = be32(bytes 0..3).  GCM's x^i is
// then bit 127 - i, and multiplying by x is a shift right.
struct Gf128 {
  uint32_t w[4];
};

// z ^ (x & m) in one v_bitop3_b32
GVS_AE_FN uint32_t xor_and(uint32_t z, uint32_t x, uint32_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_bitop3_b32(z, x, m, 0x78);
#else
  return z ^ (x & m);
#endif
}

// a * b in GF(2^128) mod x^128 + x^7 + x^2 + x + 1.  Step i adds a << i into
// the 256-bit product once per word of b, under the mask of that word's bit
// i: 29 operations for four multiplier bits.  The bit-reversed product of two
// 128-bit integers sits one bit low in 256 bits; after the shift that puts it
// right the low half folds into the high half word by word.
GVS_AE_FN Gf128 gf128_mul(const Gf128& a, const Gf128& b) {
  uint32_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t x0 = a.w[0], x1 = a.w[1], x2 = a.w[2], x3 = a.w[3], x4 = 0;
#pragma unroll 2
  for (uint32_t i = 0; i < 32; ++i) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const uint32_t m = 0u - ((b.w[w] >> i) & 1u);
      z[w] = xor_and(z[w], x0, m);
      z[w + 1] = xor_and(z[w + 1], x1, m);
      z[w + 2] = xor_and(z[w + 2], x2, m);
      z[w + 3] = xor_and(z[w + 3], x3, m);
      z[w + 4] = xor_and(z[w + 4], x4, m);
    }
    x4 = (x4 << 1) | (x3 >> 31);
    x3 = (x3 << 1) | (x2 >> 31);
    x2 = (x2 << 1) | (x1 >> 31);
    x1 = (x1 << 1) | (x0 >> 31);
    x0 <<= 1;
  }
#pragma unroll
  for (int k = 7; k > 0; --k) z[k] = (z[k] << 1) | (z[k - 1] >> 31);
  z[0] <<= 1;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t lw = z[i];
    z[i + 4] ^= lw ^ (lw >> 1) ^ (lw >> 2) ^ (lw >> 7);
    z[i + 3] ^= (lw << 31) ^ (lw << 30) ^ (lw << 25);
  }
  return Gf128{{z[4], z[5], z[6], z[7]}};
}

// a 16-byte block held as four little-endian memory words <-> the element
GVS_AE_FN Gf128 gf128_of_block(uint4 d) {
  return Gf128{{bswap32(d.w), bswap32(d.z), bswap32(d.y), bswap32(d.x)}};
}

// ------------------------------------------------------------------ serial form

inline uint32_t ae_be32(const uint8_t* p) {
  return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3];
}

// One message on the host, block after block, from the same primitives: the
// checker of the wave form and what the CPU tests run.  seal: out = C | tag
// (len + 16 bytes), returns true.  open: in = C | tag; out = P (len - 16
// bytes); a short message or a wrong tag returns false and zeroes out.
inline bool aead_serial(bool seal, const uint32_t* te0, const uint8_t key[32], const uint8_t iv[12],
                        const uint8_t* aad, uint32_t aad_len, const uint8_t* in, uint32_t in_len,
                        uint8_t* out) {
  if (!seal && in_len < kAeadTag) return false;
  const uint32_t len = seal ? in_len : in_len - kAeadTag;
  uint32_t kw[8], w[60];
  for (int i = 0; i < 8; ++i) kw[i] = ae_be32(key + 4 * i);
  aes256_expand(te0, kw, w);
  uint4 rk[15];
  for (int r = 0; r < 15; ++r) rk[r] = make_uint4(w[4 * r], w[4 * r + 1], w[4 * r + 2], w[4 * r + 3]);
  const uint32_t iw[3] = {ae_be32(iv), ae_be32(iv + 4), ae_be32(iv + 8)};
  uint32_t hb[4] = {0, 0, 0, 0}, ej[4] = {iw[0], iw[1], iw[2], 1};
  aes256_encrypt2(rk, te0, hb, ej);
  const Gf128 H{{hb[3], hb[2], hb[1], hb[0]}};
  Gf128 y{{0, 0, 0, 0}};
  auto absorb = [&](const uint8_t* p, uint32_t n) {  // n bytes, the last block zero-padded
    for (uint32_t o = 0; o < n; o += 16) {
      uint8_t blk[16] = {};
      for (uint32_t k = 0; k < 16 && o + k < n; ++k) blk[k] = p[o + k];
      for (int k = 0; k < 4; ++k) y.w[3 - k] ^= ae_be32(blk + 4 * k);
      y = gf128_mul(y, H);
    }
  };
  absorb(aad, aad_len);
  if (!seal) absorb(in, len);
  for (uint32_t o = 0; o < len; o += 32) {  // two counter blocks per call
    uint32_t ca[4] = {iw[0], iw[1], iw[2], o / 16 + 2}, cb[4] = {iw[0], iw[1], iw[2], o / 16 + 3};
    aes256_encrypt2(rk, te0, ca, cb);
    for (uint32_t k = 0; k < 32 && o + k < len; ++k) {
      const uint32_t* ks = k < 16 ? ca : cb;
      out[o + k] = in[o + k] ^ (uint8_t)(ks[(k & 15) >> 2] >> (24 - 8 * (k & 3)));
    }
  }
  if (seal) absorb(out, len);
  y.w[2] ^= aad_len * 8u;
  y.w[0] ^= len * 8u;
  y = gf128_mul(y, H);
  uint8_t tag[16];
  for (int k = 0; k < 16; ++k) tag[k] = (uint8_t)((y.w[3 - (k >> 2)] ^ ej[k >> 2]) >> (24 - 8 * (k & 3)));
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

struct AeadArgs {
  const uint4* keys;         // n x 32 B
  const uint32_t* ivs;       // n x 12 B
  const uint8_t* aad;        // message i's AAD at aad + i * aad_stride; null: no AAD
  uint32_t aad_stride;
  const uint32_t* aad_lens;
  const uint8_t* in;         // seal: P; open: C | tag
  uint32_t in_stride;
  const uint32_t* in_lens;
  uint32_t n;
  uint8_t* out;              // seal: C | tag; open: P; every slot written whole
  uint32_t out_stride;
  uint32_t* out_lens;
  uint32_t* ok;              // per-message verdict (optional for seal)
  const uint32_t* te;        // the 256-word AES table
  // the channel wire call's merge (seal only; both null otherwise): a message
  // whose request did not open (opened[i] = 0) gets status[i] = bad_status and,
  // like an empty response, is not sealed: out_lens[i] = 0, a zeroed slot
  const uint32_t* opened;
  uint32_t* status;
  uint32_t bad_status;
};

#if defined(__HIPCC__)

// Per-wave LDS, in the holes of the AES table's window (bytes [128, 256) of
// every 256-B entry row, gvs_seal_dev.h): 512 16-byte cells per wave.
constexpr uint32_t kAeCells = 512;
constexpr uint32_t kAeRk = 0;     // 15 round keys
constexpr uint32_t kAeHp = 16;    // H^1 .. H^64
constexpr uint32_t kAeX = 80;     // the hash input: AAD blocks, C blocks, the length block (<= 133)
constexpr uint32_t kAeY = 216;    // open: the plaintext blocks (<= 128)
static_assert(kAeY + kAeadTextMax / 16 <= kAeCells, "a wave's cells");
static_assert(kAeX + kAeadAadMax / 16 + kAeadTextMax / 16 + 1 <= kAeY, "the hash input");
static_assert(kAeadMsgs * kAeCells * 16 <= 256 * 128, "the window's holes");

// cell i: eight to a hole, so consecutive cells are not consecutive addresses
__device__ inline uint4* ae_cell(uint32_t* s_te, uint32_t i) {
  return reinterpret_cast<uint4*>(reinterpret_cast<char*>(s_te) + (i >> 3) * 256u + 128u + (i & 7u) * 16u);
}

// the wave's round keys
struct AeRk {
  uint32_t* s_te;
  uint32_t base;
  __device__ uint4 operator[](int r) const { return *ae_cell(s_te, base + (uint32_t)r); }
};

// the first nbytes bytes (as a signed count: <= 0 none, >= 16 all) of a block
// of little-endian memory words
__device__ inline uint4 ae_keep(uint4 v, int nbytes) {
  uint32_t m[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = nbytes - 4 * k;
    m[k] = r >= 4 ? ~0u : (r <= 0 ? 0u : (1u << (8 * (r & 3))) - 1u);
  }
  return make_uint4(v.x & m[0], v.y & m[1], v.z & m[2], v.w & m[3]);
}

__device__ inline Gf128 ae_ld_gf(const uint4* p) {
  const uint4 d = *p;
  return Gf128{{d.x, d.y, d.z, d.w}};
}

// One wave per message, four messages per workgroup; the grid follows n only.
//  1. the wave expands its key (every lane the same words, lane 0 stores them)
//     into LDS; round-key reads are broadcasts from then on
//  2. CTR, two blocks per lane per pass: virtual block v = 128 pass + lane
//     (+ 64) is E_K(0) for v = 0, E_K(IV | 1) for v = 1 and keystream block
//     v - 2 otherwise, so the hash key and the tag mask cost no AES pass of
//     their own.  The hash input (always ciphertext) goes to LDS at its GHASH
//     position, an opened message's plaintext beside it
//  3. H^1 .. H^min(64, m) by log-step doubling: step s gives lanes [2^s, 2^(s+1))
//     H^(2^s) * H^(lane + 1 - 2^s)
//  4. GHASH in chunks of 64 blocks: lane l multiplies block l (lane 0's with
//     the running value folded in) by H^(cnt - l), and a shuffle butterfly
//     XORs the 64 products
//  5. open: the tag is compared bytewise in lanes 0..15 and OR-folded by a
//     ballot; output blocks are (text & verdict), all out_stride / 16 of them
template <bool SEAL>
__global__ void __launch_bounds__(64 * kAeadMsgs) k_aead(AeadArgs a) {
  GVS_TE_LDS s_te[kTeWords];
  load_te(s_te, a.te);
  __syncthreads();
  const uint32_t lane = lane_id();
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t i = blockIdx.x * kAeadMsgs + wave;
  if (i >= a.n) return;
  const LdsTe te = lds_te(s_te);
  const uint32_t cb = wave * kAeCells;

  // lengths: uniform, and the only data that loops and addresses follow
  const uint32_t in_len = __builtin_amdgcn_readfirstlane(a.in_lens[i]);
  uint32_t aad_len = a.aad ? __builtin_amdgcn_readfirstlane(a.aad_lens[i]) : 0u;
  const bool merge = SEAL && a.opened != nullptr;
  bool len_ok = in_len <= a.in_stride && aad_len <= kAeadAadMax && aad_len <= a.aad_stride;
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
  const uint32_t m = na + nc + 1u;  // hash blocks

  // 1. the key schedule
  {
    const uint4 k0 = a.keys[2 * (uint64_t)i], k1 = a.keys[2 * (uint64_t)i + 1];
    const uint32_t kw[8] = {bswap32(k0.x), bswap32(k0.y), bswap32(k0.z), bswap32(k0.w),
                            bswap32(k1.x), bswap32(k1.y), bswap32(k1.z), bswap32(k1.w)};
    uint32_t w[60];
    aes256_expand(te, kw, w);
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < 15; ++r)
        *ae_cell(s_te, cb + kAeRk + r) = make_uint4(w[4 * r], w[4 * r + 1], w[4 * r + 2], w[4 * r + 3]);
    }
  }
  // the hash input's AAD blocks and length block
  const uint8_t* aadp = a.aad + (uint64_t)i * a.aad_stride;
  if (lane < na) {
    const uint4 d = *reinterpret_cast<const uint4*>(aadp + 16u * lane);
    *ae_cell(s_te, cb + kAeX + lane) = ae_keep(d, (int)aad_len - 16 * (int)lane);
  }
  if (lane == 0)
    *ae_cell(s_te, cb + kAeX + na + nc) = make_uint4(0u, bswap32(aad_len * 8u), 0u, bswap32(text_len * 8u));
  wave_lds_sync();

  // 2. CTR
  const AeRk rk{s_te, cb + kAeRk};
  const uint32_t* ivp = a.ivs + 3 * (uint64_t)i;
  const uint32_t iv0 = bswap32(ivp[0]), iv1 = bswap32(ivp[1]), iv2 = bswap32(ivp[2]);
  const uint8_t* inp = a.in + (uint64_t)i * a.in_stride;
  uint32_t hw[4] = {0, 0, 0, 0}, ej[4] = {0, 0, 0, 0};
  const uint32_t npass = (nc + 2u + 127u) / 128u;
  for (uint32_t p = 0; p < npass; ++p) {
    const uint32_t v0 = 128u * p + lane, v1 = v0 + 64u;
    const bool z = v0 == 0;  // the hash key's block is all zero
    uint32_t sa[4] = {z ? 0u : iv0, z ? 0u : iv1, z ? 0u : iv2, v0};
    uint32_t sb[4] = {iv0, iv1, iv2, v1};
    aes256_encrypt2(rk, te, sa, sb);
    if (p == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        hw[k] = __shfl(sa[k], 0);
        ej[k] = __shfl(sa[k], 1);
      }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint32_t t = (h ? v1 : v0) - 2u;  // text block; wraps past nc for v < 2
      const uint32_t* ks = h ? sb : sa;
      if (t < nc) {
        const uint4 d = *reinterpret_cast<const uint4*>(inp + 16u * t);
        const int nb = (int)text_len - 16 * (int)t;
        const uint4 o = ae_keep(make_uint4(d.x ^ bswap32(ks[0]), d.y ^ bswap32(ks[1]),
                                           d.z ^ bswap32(ks[2]), d.w ^ bswap32(ks[3])), nb);
        *ae_cell(s_te, cb + kAeX + na + t) = SEAL ? o : ae_keep(d, nb);
        if (!SEAL) *ae_cell(s_te, cb + kAeY + t) = o;
      }
    }
  }

  // 3. the powers of H
  const Gf128 H{{hw[3], hw[2], hw[1], hw[0]}};
  if (lane == 0) *ae_cell(s_te, cb + kAeHp) = make_uint4(H.w[0], H.w[1], H.w[2], H.w[3]);
  const uint32_t maxp = m < 64u ? m : 64u;
  for (uint32_t step = 1; step < maxp; step <<= 1) {
    wave_lds_sync();
    const Gf128 top = ae_ld_gf(ae_cell(s_te, cb + kAeHp + step - 1u));
    const Gf128 low = ae_ld_gf(ae_cell(s_te, cb + kAeHp + ((lane - step) & (step - 1u))));
    const Gf128 pr = gf128_mul(top, low);
    if (lane >= step && lane < 2u * step)
      *ae_cell(s_te, cb + kAeHp + lane) = make_uint4(pr.w[0], pr.w[1], pr.w[2], pr.w[3]);
  }
  wave_lds_sync();

  // 4. GHASH
  Gf128 y{{0, 0, 0, 0}};
  for (uint32_t c0 = 0; c0 < m; c0 += 64u) {
    const uint32_t cnt = m - c0 < 64u ? m - c0 : 64u;
    const bool live = lane < cnt;
    const uint4 d = *ae_cell(s_te, cb + kAeX + (live ? c0 + lane : 0u));
    Gf128 blk = gf128_of_block(d);
    const bool first = lane == 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) blk.w[k] = live ? blk.w[k] ^ (first ? y.w[k] : 0u) : 0u;
    const Gf128 hp = ae_ld_gf(ae_cell(s_te, cb + kAeHp + ((cnt - 1u - lane) & 63u)));
    Gf128 pr = gf128_mul(blk, hp);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
      for (int k = 0; k < 4; ++k) pr.w[k] ^= __shfl_xor(pr.w[k], off);
    }
    y = pr;
  }
  const uint32_t tg[4] = {y.w[3] ^ ej[0], y.w[2] ^ ej[1], y.w[1] ^ ej[2], y.w[0] ^ ej[3]};
  // tag byte lane & 15
  const uint32_t tq = (lane >> 2) & 3u;
  const uint32_t tword = tq == 0 ? tg[0] : tq == 1 ? tg[1] : tq == 2 ? tg[2] : tg[3];
  const uint32_t tbyte = (tword >> (24u - 8u * (lane & 3u))) & 0xffu;

  // 5. the verdict and the output slot
  bool emit = len_ok;
  if (SEAL) {
    if (merge) emit = emit & (a.opened[i] != 0);
  } else {
    const uint32_t theirs = inp[text_len + (lane & 15u)];  // in_stride >= 16 whatever the length
    const bool differs = (lane < 16u) & (theirs != tbyte);
    emit = emit & (__ballot(differs) == 0);
  }
  const uint32_t keep = emit ? ~0u : 0u;
  uint8_t* outp = a.out + (uint64_t)i * a.out_stride;
  for (uint32_t b = lane; b < a.out_stride / 16u; b += 64u) {
    const bool src = b < nc;
    const uint4 d = *ae_cell(s_te, cb + (SEAL ? kAeX + na : kAeY) + (src ? b : 0u));
    const uint32_t kb = src ? keep : 0u;
    *reinterpret_cast<uint4*>(outp + 16u * b) = make_uint4(d.x & kb, d.y & kb, d.z & kb, d.w & kb);
  }
  if (SEAL) {
    // the tag follows the text at any byte offset: byte stores, after the
    // block stores they overlap
    __threadfence_block();
    if (lane < 16u) outp[text_len + lane] = (uint8_t)(tbyte & keep);
  }
  if (lane == 0) {
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
