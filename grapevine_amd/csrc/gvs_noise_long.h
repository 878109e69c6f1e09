// gvs_noise_long.h — the end of the Noise IX responder's chain for a message-2
// payload of up to 65 439 bytes (message 2 <= 65 535, Noise's limit):
// k_noise_ix_tail does MixHash(ct_p), Split and the assembly of message 2 that
// k_noise_ix<C> does for short payloads.
//
// One lane per handshake, 64 handshakes per wavefront, k_noise_hkdf's launch
// shape: a SHA-512 chain over one message is serial, so a quad's other lanes
// could only idle through its up to 513 blocks.  One rolled loop around one
// inlined copy of the rounds; step t < nb hashes block t of H(h | ct_p), the
// twelve steps after it are noise_hkdf_one's schedule with an empty input.
//
// ct_p is k_aead_long's output: 16-byte-aligned rows, up16(p2 + 16) apart, zero
// from the tag's end to the stride.  A lane loads a block as eight 16-byte
// words (block 0: h from the state row, then the first 64 bytes) and swaps
// bytes in registers; block t + 1 is loaded before block t's rounds start.
// What it has loaded it stores, ANDed with the handshake's verdict, to message
// 2 at 80 + the row offset; after the loop come the header (e_pub | ct_s) and
// zeros to the end of the slot, so the slot is written whole, once, by the
// same stores whether the handshake holds or not.  The 0x80 and the bit count
// are ORed into the words that p2 places them in.
//
// What depends on data: p2 and the strides alone (the same for every lane)
// reach branches, trip counts and addresses.  The verdict (message 1's length
// check and k_x25519's three flags) is known before the loop and is a mask;
// h, ck, ct_p and the keys reach no branch and no address.
//
// nt_item is host/device code: tests/noise_long_host.cpp runs it in a loop
// over the handshakes, k_noise_ix_tail runs it in a lane.
#pragma once
#include "gvs_aead_long.h"
#include "gvs_noise.h"

namespace gvs {
namespace sr {

constexpr uint32_t kNxPayload2LongMax = 65439;  // GVS_NOISE_PAYLOAD2_LONG_MAX: 96 + p2 <= 65 535
constexpr uint32_t kNtSplit = 12;               // compressions of an HKDF

// the tail's trip count for a payload 2 of p2 bytes (NxArgs::steps_c)
__host__ __device__ constexpr uint32_t nt_steps(uint32_t p2) { return nx_blocks(p2 + 16u) + kNtSplit; }
// ct_p's row stride
__host__ __device__ constexpr uint32_t nt_row(uint32_t p2) { return (p2 + 16u + 15u) & ~15u; }

struct NtLane {
  uint64_t h[8];      // the running state: the transcript's, then an HMAC's
  uint64_t key[8];    // the HMAC key: ck, then temp
  uint64_t inner[8];  // an HMAC's inner digest
  uint64_t out1[8];   // o1
  uint4 nxt[8];       // the next block of the transcript, as loaded
};

GVS_SR_FN uint4 nt_and(uint4 v, uint32_t m) { return make_uint4(v.x & m, v.y & m, v.z & m, v.w & m); }

// two big-endian words of 16 loaded bytes
GVS_SR_FN void nt_be(uint4 v, uint64_t& hi, uint64_t& lo) {
  hi = (uint64_t)bswap32(v.x) << 32 | bswap32(v.y);
  lo = (uint64_t)bswap32(v.z) << 32 | bswap32(v.w);
}

// Block b of h | ct_p into L.nxt: word c is bytes [16c, 16c + 16) of the block,
// row offset 128 b - 64 + 16 c.  Past the row's end nothing is read.
GVS_SR_FN void nt_load(const uint8_t* h, const uint8_t* row, uint32_t stride, uint32_t b, NtLane& L) {
#pragma unroll
  for (uint32_t c = 0; c < 8; ++c) {
    const uint32_t o = 128u * b + 16u * c - 64u;
    if (b == 0 && c < 4)
      L.nxt[c] = al_ld(h + 16u * c);
    else if (o < stride)
      L.nxt[c] = al_ld(row + o);
    else
      L.nxt[c] = make_uint4(0u, 0u, 0u, 0u);
  }
}

// One handshake's tail.  a.steps_c = nt_steps(a.p2), a.ct2_stride =
// nt_row(a.p2); st, xout, ct1, ct2 and msg2 rows are 16-byte aligned and
// a.msg2_stride is a multiple of 16 that holds 96 + p2.
GVS_SR_FN_NI void nt_item(const NxArgs& a, uint32_t i) {
  constexpr uint64_t kIv[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull,
                               0xa54ff53a5f1d36f1ull, 0x510e527fade682d1ull, 0x9b05688c2b3e6c1full,
                               0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
  const uint32_t len1 = a.msg1_lens[i];
  const uint32_t* xk = a.xok + 4u * (uint64_t)i;
  const uint32_t good = (uint32_t)(len1 >= 64u) & (uint32_t)(len1 <= 64u + kNxPayload1Max) &
                        (uint32_t)(xk[1] != 0) & (uint32_t)(xk[2] != 0) & (uint32_t)(xk[3] != 0);
  const uint32_t vm = 0u - good;
  const uint64_t m = 0ull - (uint64_t)good;

  const uint8_t* st = a.st + 128u * (uint64_t)i;
  const uint8_t* row = a.ct2 + (uint64_t)i * a.ct2_stride;
  uint8_t* slot = a.msg2 + (uint64_t)i * a.msg2_stride;
  const uint32_t nb = nx_blocks(a.p2 + 16u);
  const uint32_t end = 64u + a.p2 + 16u;  // bytes hashed: the 0x80 goes after them
  const uint32_t end_blk = end >> 7, end_word = (end & 127u) >> 3;
  const uint64_t end_bit = 0x80ull << (56u - 8u * (end & 7u));

  NtLane L;
#pragma unroll
  for (int j = 0; j < 8; ++j) L.h[j] = L.key[j] = L.inner[j] = L.out1[j] = 0;
  nt_load(st + 64, row, a.ct2_stride, 0u, L);

#pragma unroll 1
  for (uint32_t t = 0; t < a.steps_c; ++t) {
    uint64_t w[16], s[8];
    if (t < nb) {  // block t of the transcript
#pragma unroll
      for (uint32_t c = 0; c < 8; ++c) {
        nt_be(L.nxt[c], w[2 * c], w[2 * c + 1]);
        const uint32_t at = 128u * t + 16u * c + 16u;  // 80 + the row offset
        if ((t != 0 || c >= 4) && at + 16u <= a.msg2_stride) al_st(slot + at, nt_and(L.nxt[c], vm));
      }
      if (t + 1u < nb) nt_load(st + 64, row, a.ct2_stride, t + 1u, L);
#pragma unroll
      for (uint32_t j = 0; j < 16; ++j) w[j] |= (t == end_blk && j == end_word) ? end_bit : 0ull;
      w[15] |= t + 1u == nb ? (uint64_t)end * 8u : 0ull;
      if (t == 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) L.h[j] = kIv[j];
      }
    } else {  // the Split: noise_hkdf_one's step c with an empty input
      const uint32_t c = t - nb, stage = c & 3u, mac = c >> 2;
      if (c == 0) {  // ck
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) nt_be(al_ld(st + 16u * j), L.key[2 * j], L.key[2 * j + 1]);
      }
#pragma unroll
      for (int j = 0; j < 16; ++j) w[j] = 0;
      if (stage == 0 || stage == 2) {
        const uint64_t pad = stage == 0 ? kNxIpad : kNxOpad;
#pragma unroll
        for (int j = 0; j < 8; ++j) w[j] = L.key[j] ^ pad, w[8 + j] = pad, L.h[j] = kIv[j];
      } else if (stage == 3) {
#pragma unroll
        for (int j = 0; j < 8; ++j) w[j] = L.inner[j];
        w[8] = kNxEnd;
        w[15] = 192u * 8u;
      } else if (mac == 0) {
        w[0] = kNxEnd;
        w[15] = 128u * 8u;
      } else if (mac == 1) {
        w[0] = 0x0180ull << 48;
        w[15] = 129u * 8u;
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) w[j] = L.out1[j];
        w[8] = 0x0280ull << 48;
        w[15] = 193u * 8u;
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = L.h[j];
    sha512_rounds<0>(s, w);
#pragma unroll
    for (int j = 0; j < 8; ++j) L.h[j] += s[j];
    if (t + 1u == nb && a.hashes) nx_st64(a.hashes + 64u * (uint64_t)i, L.h, 8, m);  // the handshake hash
    if (t >= nb) {
      const uint32_t c = t - nb;
      if ((c & 3u) == 1u) {
#pragma unroll
        for (int j = 0; j < 8; ++j) L.inner[j] = L.h[j];
      }
      if (c == 3u) {
#pragma unroll
        for (int j = 0; j < 8; ++j) L.key[j] = L.h[j];  // temp
      }
      if (c == 7u) {
#pragma unroll
        for (int j = 0; j < 8; ++j) L.out1[j] = L.h[j];
      }
    }
  }

  nx_st64(a.recv + 32u * (uint64_t)i, L.out1, 4, m);  // k1 = o1[0:32]
  nx_st64(a.send + 32u * (uint64_t)i, L.h, 4, m);     // k2 = o2[0:32]
  a.ok[i] = good;
  a.msg2_lens[i] = good ? kNxMsg2Fixed + a.p2 : 0u;
  // the header, and zeros from the last block's end to the end of the slot
  const uint8_t *ep = a.xout + 128u * (uint64_t)i, *c1 = a.ct1 + 48u * (uint64_t)i;
#pragma unroll
  for (uint32_t c = 0; c < 5; ++c) al_st(slot + 16u * c, nt_and(al_ld(c < 2 ? ep + 16u * c : c1 + 16u * (c - 2u)), vm));
  for (uint32_t at = 128u * nb + 16u; at < a.msg2_stride; at += 16u) al_st(slot + at, make_uint4(0u, 0u, 0u, 0u));
}

#if defined(__HIPCC__)

__global__ void __launch_bounds__(kSrThreads) k_noise_ix_tail(NxArgs a) {
  const uint32_t k = blockIdx.x * kSrThreads + threadIdx.x;
  if (k < a.n) nt_item(a, k);
}

// One payload for all (payload_stride = 0) as k_aead_long's text rows: the
// kernel refuses a message longer than its in_stride, so it cannot read a
// shared payload in place.  A thread per 16-byte word; only the payload's last,
// partial word is put together from bytes.
struct NxSpreadArgs {
  const uint8_t* payload;  // p2 bytes, 16-byte aligned
  uint32_t p2, stride, n;  // stride = up16(p2)
  uint8_t* text2;          // n rows
};

__global__ void __launch_bounds__(256) k_noise_ix_spread(NxSpreadArgs a) {
  const uint32_t per = a.stride / 16u;
  const uint64_t x = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (x >= (uint64_t)a.n * per) return;
  const uint32_t o = 16u * (uint32_t)(x % per);
  uint4 v;
  if (o + 16u <= a.p2) {
    v = al_ld(a.payload + o);
  } else {
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k)
      if (o + k < a.p2) w[k >> 2] |= (uint32_t)a.payload[o + k] << (8u * (k & 3u));
    v = make_uint4(w[0], w[1], w[2], w[3]);
  }
  al_st(a.text2 + 16u * x, v);
}

#endif  // __HIPCC__

}  // namespace sr
}  // namespace gvs
