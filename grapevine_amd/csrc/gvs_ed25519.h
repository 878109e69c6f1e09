// gvs_ed25519.h — gfx950 kernel of the challenge check for deployments whose
// clients hold Ed25519 keys (README.md of the reference: the record's key
// fields are ristretto points, and the service "could compile it to use
// ed25519 instead").  Pure Ed25519 (RFC 8032 §5.1), verified in batch before
// the store sees the requests, on the field, curve and scalar code of
// gvs_sr25519.h.
//
// Verify(pk, msg, sig = R || s), the rule of oracle/sr25519.py::ed25519_verify
// [D: RFC 8032 strict decoding, cofactorless; not ed25519-dalek's legacy
// acceptance rules]:
//   s < l; A = decode(pk) strictly (y < p, x^2 a square, not x = 0 with the
//   sign bit set); h = SHA-512(R || pk || msg) mod l;
//   accept iff encode(s*B - h*A) == R byte for byte.
// The encoder emits only the canonical encoding of a curve point, so the byte
// comparison is the oracle's "R decodes strictly and s*B == R + h*A" without a
// decode of R.  There is no small-order test.
//
// One thread per signature, the launch shape of k_sr_verify.  SHA-512 keeps
// its 16-word schedule window and 8 working variables in registers (every
// index a compile-time constant); its trip count and every branch inside it
// depend on msg_len alone, a kernel argument.  The digest, then the
// per-signature -A table, live in the thread's LDS column.  No branch, loop
// bound or address depends on key, message or signature bytes.
#pragma once
#include "gvs_sr25519.h"

namespace gvs {
namespace sr {

// ------------------------------------------------------------------ SHA-512

// FIPS 180-4 §4.2.3
__host__ __device__ constexpr uint64_t sha512_k(int t) {
  constexpr uint64_t K[80] = {
      0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull,
      0x3956c25bf348b538ull, 0x59f111f1b605d019ull, 0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull,
      0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull,
      0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull, 0xc19bf174cf692694ull,
      0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull,
      0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull,
      0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull,
      0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull, 0x06ca6351e003826full, 0x142929670a0e6e70ull,
      0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull, 0x53380d139d95b3dfull,
      0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull,
      0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull, 0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull,
      0xd192e819d6ef5218ull, 0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull,
      0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull,
      0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull,
      0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
      0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull,
      0xca273eceea26619cull, 0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull,
      0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull, 0x113f9804bef90daeull, 0x1b710b35131c471bull,
      0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull, 0x431d67c49c100d4cull,
      0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull};
  return K[t];
}

GVS_SR_FN uint64_t sha512_rotr(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }

// Round T with compile-time indices: working variable a..h is s[(i - T) & 7]
// (the rotation of the eight is a renaming, not a move) and the schedule is a
// 16-word window, so both arrays stay in registers and the round constant is
// an immediate.
template <int T>
GVS_SR_FN void sha512_round(uint64_t (&s)[8], uint64_t (&w)[16]) {
  if constexpr (T >= 16) {
    const uint64_t w15 = w[(T - 15) & 15], w2 = w[(T - 2) & 15];
    w[T & 15] += (sha512_rotr(w15, 1) ^ sha512_rotr(w15, 8) ^ (w15 >> 7)) + w[(T - 7) & 15] +
                 (sha512_rotr(w2, 19) ^ sha512_rotr(w2, 61) ^ (w2 >> 6));
  }
  const uint64_t a = s[(0 - T) & 7], b = s[(1 - T) & 7], c = s[(2 - T) & 7];
  const uint64_t e = s[(4 - T) & 7], f = s[(5 - T) & 7], g = s[(6 - T) & 7];
  constexpr uint64_t k = sha512_k(T);
  const uint64_t t1 = s[(7 - T) & 7] + (sha512_rotr(e, 14) ^ sha512_rotr(e, 18) ^ sha512_rotr(e, 41)) +
                      ((e & f) ^ (~e & g)) + k + w[T & 15];
  const uint64_t t2 = (sha512_rotr(a, 28) ^ sha512_rotr(a, 34) ^ sha512_rotr(a, 39)) +
                      ((a & b) ^ (a & c) ^ (b & c));
  s[(3 - T) & 7] += t1;
  s[(7 - T) & 7] = t1 + t2;
}

template <int T>
GVS_SR_FN void sha512_rounds(uint64_t (&s)[8], uint64_t (&w)[16]) {
  if constexpr (T < 80) {
    sha512_round<T>(s, w);
    sha512_rounds<T + 1>(s, w);
  }
}

// The hashed string: three pieces end to end (R, A and M for a signature).
// The lengths are the same in every thread of a launch.
struct Sha512In {
  const uint8_t* p0;
  uint32_t n0;
  const uint8_t* p1;
  uint32_t n1;
  const uint8_t* p2;
  uint32_t n2;
};

// Byte `pos` of the padded message (FIPS 180-4 §5.1.2) without its length
// field; pos and the lengths are uniform, so these are scalar branches
GVS_SR_FN uint64_t sha512_byte(const Sha512In& in, uint32_t pos) {
  const uint32_t e0 = in.n0, e1 = e0 + in.n1, e2 = e1 + in.n2;
  uint32_t v = 0;
  if (pos < e0)
    v = in.p0[pos];
  else if (pos < e1)
    v = in.p1[pos - e0];
  else if (pos < e2)
    v = in.p2[pos - e1];
  else if (pos == e2)
    v = 0x80u;
  return v;
}

// SHA-512 of the three pieces; digest byte j is byte j & 3 of out[(j >> 2) *
// stride] (the little-endian words sc_reduce_wide reads).  Any number of
// 128-byte blocks: the trip count depends on the total length alone.
GVS_SR_FN_NI void sha512_3(const Sha512In& in, uint32_t* out, uint32_t stride) {
  uint64_t h[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull,
                   0xa54ff53a5f1d36f1ull, 0x510e527fade682d1ull, 0x9b05688c2b3e6c1full,
                   0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
  const uint32_t total = in.n0 + in.n1 + in.n2;
  const uint32_t blocks = (total + 1u + 16u + 127u) >> 7;  // 0x80, the 128-bit length
  for (uint32_t blk = 0; blk < blocks; ++blk) {
    uint64_t w[16], s[8];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      uint64_t x = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) x = (x << 8) | sha512_byte(in, blk * 128u + 8u * i + j);
      w[i] = x;
    }
    // the last block ends with the length in bits (below 2^64: w[14] stays 0)
    w[15] |= blk + 1u == blocks ? (uint64_t)total * 8u : 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] = h[i];
    sha512_rounds<0>(s, w);
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] += s[i];
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {  // big-endian 64-bit words -> little-endian 32-bit words
    out[(2 * i) * stride] = __builtin_bswap32((uint32_t)(h[i] >> 32));
    out[(2 * i + 1) * stride] = __builtin_bswap32((uint32_t)h[i]);
  }
}

// ------------------------------------------------------------ edwards25519

// z^-1 = z^(p - 2) = (z^(2^252 - 3))^8 * z^3   (0 for z = 0)
GVS_SR_FN_NI Fe fe_invert(const Fe& z) {
  const Fe z3 = fe_mul(fe_sq(z), z);
  return fe_mul(fe_sqn(fe_pow22523(z), 3), z3);
}

// RFC 8032 §5.1.3, strict: *ok all ones when b (32 bytes as 8 little-endian
// words) is y < p with a square x^2 = (y^2 - 1) / (d y^2 + 1), and not x = 0
// with the sign bit set.  The same rule as oracle/sr25519.py::_ed_decode.
GVS_SR_FN_NI Pt ed_decode(const Fe& b, uint32_t* ok) {
  const uint32_t sign = 0u - (b.v[7] >> 31);
  Fe y = b;
  y.v[7] &= 0x7FFFFFFFu;
  const Fe p = fe_p();
  uint64_t t = 0;  // y < p
#pragma unroll
  for (int i = 0; i < 8; ++i) t = (uint64_t)y.v[i] - p.v[i] - ((t >> 32) & 1u);
  const uint32_t canonical = 0u - ((uint32_t)(t >> 32) & 1u);
  const Fe yy = fe_sq(y);
  const Fe u = fe_sub(yy, fe_one()), v = fe_add(fe_mul(fe_d(), yy), fe_one());
  uint32_t was_square;
  Fe x = fe_sqrt_ratio_m1(u, v, &was_square);  // the non-negative (even) root
  const uint32_t x_zero = fe_mask_eq(x, fe_zero());
  *ok = canonical & was_square & ~(x_zero & sign);
  x = fe_select(sign, fe_neg(x), x);
  return Pt{x, y, fe_one(), fe_mul(x, y)};
}

// RFC 8032 §5.1.2: the canonical y with x's parity in bit 255
GVS_SR_FN_NI Fe ed_encode(const Pt& q) {
  const Fe zi = fe_invert(q.Z);
  const Fe x = fe_canon(fe_mul(q.X, zi));
  Fe y = fe_canon(fe_mul(q.Y, zi));
  y.v[7] |= (x.v[0] & 1u) << 31;
  return y;
}

// One signature: all ones if valid.  col: this thread's 128-word column
// (stride ts) for the digest and then the -A table; btab: {B, 2B, 3B, 4B}
// cached (ptc_table4).
GVS_SR_FN_NI uint32_t ed_verify_one(const uint8_t* pk, const uint8_t* msg, uint32_t msg_len,
                                    const uint8_t* sig, uint32_t* col, uint32_t ts,
                                    const uint32_t* btab) {
  sha512_3(Sha512In{sig, 32u, pk, 32u, msg, msg_len}, col, ts);
  const Fe hc = sc_reduce_wide(col, ts);
  Fe sc, A_s, R_s;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    sc.v[i] = ld_le32(sig + 32 + 4 * i);
    A_s.v[i] = ld_le32(pk + 4 * i);
    R_s.v[i] = ld_le32(sig + 4 * i);
  }
  uint32_t ok = sc_mask_lt_l(sc);
  uint32_t pk_ok;
  const Pt A = ed_decode(A_s, &pk_ok);
  ok &= pk_ok;
  const Fe enc = ed_encode(double_scalar_mul(sc, hc, A, col, ts, btab));
  uint32_t diff = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) diff |= enc.v[i] ^ R_s.v[i];
  return ok & (0u - (uint32_t)(diff == 0));
}

// Host form (tests/ed_host.cpp): the column and the B table in local arrays.
inline uint32_t ed_verify_host(const uint8_t* pk, const uint8_t* msg, uint32_t msg_len,
                               const uint8_t* sig) {
  uint32_t col[128], btab[128];
  ptc_table4(btab, 1, pt_base());
  return ed_verify_one(pk, msg, msg_len, sig, col, 1, btab);
}

struct EdArgs {             // SrArgs without the signing context
  const uint8_t* pk;        // n public keys, pk_stride bytes apart
  uint32_t pk_stride;
  const uint8_t* msg;       // n messages of msg_len bytes, msg_stride apart
  uint32_t msg_stride, msg_len;
  const uint8_t* sig;       // n 64-B signatures, sig_stride apart
  uint32_t sig_stride, n;
  uint32_t* ok;             // n: 1 valid, 0 invalid (may be null)
  uint4* reqs;              // optional gvs_request slab: an invalid signature sets type 0
  uint32_t* status;         // optional per-request wire status: 0 -> 3 on a bad signature
};

__global__ void __launch_bounds__(kSrThreads) k_ed_verify(EdArgs a) {
  // per thread: the digest (16 words), then this signature's -A table (128
  // words); plus the B table, shared
  __shared__ uint32_t cols[128 * kSrThreads];
  __shared__ uint32_t btab[128];
  if (threadIdx.x == 0) ptc_table4(btab, 1, pt_base());
  __syncthreads();
  const uint32_t tid = threadIdx.x;
  const uint32_t k = blockIdx.x * kSrThreads + tid;
  const uint32_t kk = k < a.n ? k : a.n - 1;  // tail threads redo the last signature
  const uint32_t ok = ed_verify_one(a.pk + (uint64_t)kk * a.pk_stride, a.msg + (uint64_t)kk * a.msg_stride,
                                    a.msg_len, a.sig + (uint64_t)kk * a.sig_stride, cols + tid,
                                    kSrThreads, btab);
  if (k >= a.n) return;
  const uint32_t valid = ok & 1u;
  if (a.ok) a.ok[k] = valid;
  if (a.reqs) {  // the request's type word: unchanged if valid, 0 (a hard error) if not
    uint4* r = a.reqs + (uint64_t)k * 65u + 64u;
    uint4 v = *r;
    v.x = valid ? v.x : 0u;
    *r = v;
  }
  if (a.status) {
    const uint32_t st = a.status[k];
    a.status[k] = (st == 0 && !valid) ? kWireBadSignature : st;
  }
}

}  // namespace sr
}  // namespace gvs
