// gvs_chacha.h — the per-connection challenge stream on the device.
//
// The reference gives every attested connection a 32-byte seed; request i on
// that connection signs bytes [32i, 32i+32) of ChaCha20Rng(seed) (README.md
// of the reference, "challenge RNG"; rand_chacha: 20 rounds, a 64-bit block
// counter from 0, stream 0).  One 64-byte block serves two draws, so
//   challenge(seed, i) = block(seed, i >> 1)[32 * (i & 1) :][:32],
// a pure function of (seed, i): one thread per request, no state on the
// device.  grapevine_amd/server.py::chacha20_block is the same function in
// Python and the checker of tests/test_chacha_host.py.
//
// State layout (rand_chacha's; RFC 8439's with the 32-bit counter and 96-bit
// nonce read as two 64-bit words):
//   words 0..3   "expand 32-byte k"
//   words 4..11  the key (seed), little-endian
//   words 12,13  block counter lo, hi
//   words 14,15  stream id lo, hi
//
// The 16 state words are 16 named registers: every index is a compile-time
// constant, so nothing is spilled to scratch.  No branch, loop bound or
// address depends on seed or draw index.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gvs {

#define GVS_CC_FN __host__ __device__ __forceinline__

constexpr uint32_t kChallengeThreads = 256;

#define GVS_CC_QR(a, b, c, d)                \
  a += b; d = __builtin_rotateleft32(d ^ a, 16); \
  c += d; b = __builtin_rotateleft32(b ^ c, 12); \
  a += b; d = __builtin_rotateleft32(d ^ a, 8);  \
  c += d; b = __builtin_rotateleft32(b ^ c, 7);

// two rounds: the four columns, then the four diagonals
#define GVS_CC_DR                                                 \
  GVS_CC_QR(x0, x4, x8, x12) GVS_CC_QR(x1, x5, x9, x13)           \
  GVS_CC_QR(x2, x6, x10, x14) GVS_CC_QR(x3, x7, x11, x15)         \
  GVS_CC_QR(x0, x5, x10, x15) GVS_CC_QR(x1, x6, x11, x12)         \
  GVS_CC_QR(x2, x7, x8, x13) GVS_CC_QR(x3, x4, x9, x14)

// out = the 64-byte ChaCha20 block (16 little-endian words) of `key` at block
// `counter` of stream `stream`
GVS_CC_FN void chacha20_block(const uint32_t key[8], uint64_t counter, uint64_t stream,
                              uint32_t out[16]) {
  const uint32_t c0 = 0x61707865u, c1 = 0x3320646eu, c2 = 0x79622d32u, c3 = 0x6b206574u;
  const uint32_t n0 = (uint32_t)counter, n1 = (uint32_t)(counter >> 32);
  const uint32_t n2 = (uint32_t)stream, n3 = (uint32_t)(stream >> 32);
  uint32_t x0 = c0, x1 = c1, x2 = c2, x3 = c3;
  uint32_t x4 = key[0], x5 = key[1], x6 = key[2], x7 = key[3];
  uint32_t x8 = key[4], x9 = key[5], x10 = key[6], x11 = key[7];
  uint32_t x12 = n0, x13 = n1, x14 = n2, x15 = n3;
  GVS_CC_DR GVS_CC_DR GVS_CC_DR GVS_CC_DR GVS_CC_DR
  GVS_CC_DR GVS_CC_DR GVS_CC_DR GVS_CC_DR GVS_CC_DR
  out[0] = x0 + c0;
  out[1] = x1 + c1;
  out[2] = x2 + c2;
  out[3] = x3 + c3;
  out[4] = x4 + key[0];
  out[5] = x5 + key[1];
  out[6] = x6 + key[2];
  out[7] = x7 + key[3];
  out[8] = x8 + key[4];
  out[9] = x9 + key[5];
  out[10] = x10 + key[6];
  out[11] = x11 + key[7];
  out[12] = x12 + n0;
  out[13] = x13 + n1;
  out[14] = x14 + n2;
  out[15] = x15 + n3;
}

#undef GVS_CC_DR
#undef GVS_CC_QR

// out = draw number `draw` (32 bytes, 8 little-endian words) of
// ChaCha20Rng(key): the low or the high half of block draw >> 1, taken with
// selects
GVS_CC_FN void challenge_draw(const uint32_t key[8], uint64_t draw, uint32_t out[8]) {
  uint32_t b[16];
  chacha20_block(key, draw >> 1, 0, b);
  const bool hi = (draw & 1u) != 0;
  out[0] = hi ? b[8] : b[0];
  out[1] = hi ? b[9] : b[1];
  out[2] = hi ? b[10] : b[2];
  out[3] = hi ? b[11] : b[3];
  out[4] = hi ? b[12] : b[4];
  out[5] = hi ? b[13] : b[5];
  out[6] = hi ? b[14] : b[6];
  out[7] = hi ? b[15] : b[7];
}

struct ChallengeArgs {
  const uint4* seeds;     // n x 32 B, 16-byte aligned
  const uint64_t* draws;  // n draw indices
  uint4* out;             // n x 32 B, 16-byte aligned
  uint32_t n;
};

// One thread per request.  Tail threads (k >= n) are masked at the loads and
// the stores and run the rounds on a zero seed; the compiler folds the two
// masks into one over the body, so a wave with no live thread skips it.  The
// only branch is on k < n.
__global__ void __launch_bounds__(kChallengeThreads) k_challenge(ChallengeArgs a) {
  const uint32_t k = blockIdx.x * kChallengeThreads + threadIdx.x;
  const bool live = k < a.n;
  uint4 s0 = make_uint4(0, 0, 0, 0), s1 = s0;
  uint64_t draw = 0;
  if (live) {
    s0 = a.seeds[2 * (uint64_t)k];
    s1 = a.seeds[2 * (uint64_t)k + 1];
    draw = a.draws[k];
  }
  const uint32_t key[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
  uint32_t c[8];
  challenge_draw(key, draw, c);
  if (live) {
    a.out[2 * (uint64_t)k] = make_uint4(c[0], c[1], c[2], c[3]);
    a.out[2 * (uint64_t)k + 1] = make_uint4(c[4], c[5], c[6], c[7]);
  }
}

}  // namespace gvs
