// gvs_x25519.h — gfx950 kernels of the channel's key agreement: batched X25519
// (RFC 7748) and Noise's HKDF over HMAC-SHA-512 (two outputs), the two
// primitives that turn a handshake's DH products into the 32-byte keys
// gvs_aead_open / gvs_aead_seal take.  The reference's Auth call is a Noise
// handshake (mc-crypto-noise, x25519-dalek and hkdf in its Cargo.lock;
// README.md:177-185) [D: the suite is Noise_IX_25519_AESGCM_SHA512; the
// snapshot names the crates, not the suite string].  The message framing
// (MixHash, the encrypted static key, the attestation payload) is not here.
//
// k_x25519: out = X25519(scalar, u).  One DPP quad (four adjacent lanes) per
// scalar multiplication: an Auth batch is what a 2-ms window collects,
// hundreds to a few thousand handshakes, and one lane per item would leave
// most SIMDs empty behind ~2 800 dependent field multiplies.  A ladder step is
// three rounds in which all four lanes run the same fe_mul:
//   round 1   D*A        C*B        A*A      B*B
//   round 2   (DA+CB)^2  (DA-CB)^2  AA*BB    a24*E
//   round 3   -          x1*(..)^2  -        E*(AA + a24*E)
// so a quad runs 255 * 3 + ~265 (the inversion, in lock-step on all four
// lanes) dependent multiplies.  Lanes 0..3 of a quad hold X3, Z3, X2, Z2 (one
// field element each, plus x1); operands move with quad_perm DPP moves, eight
// per field element, five elements per step: the step's leading conditional
// swap is one of them (a select between the state and its rotation by two
// lanes).  No LDS and no ds_bpermute.
//
// Constant time (DESIGN.md §3 rules 12, 16, 17): the swap is a mask select on
// the XOR of consecutive scalar bits; the loop is rolled, 255 trips; the
// scalar is shifted left one bit per trip and read at its top bit, so no
// register array is indexed by a variable.  Nothing branches on or addresses
// by scalar, point or result.
//
// k_noise_hkdf: temp = HMAC(ck, ikm), o1 = HMAC(temp, 0x01), o2 = HMAC(temp,
// o1 || 0x02), ikm of 0 bytes (Split) or 32 (MixKey of a DH output).  Every
// HMAC is four compressions (key pad, message, key pad, inner digest), twelve
// per item, in one rolled loop around one copy of gvs_ed25519.h's rounds.  One
// thread per item, the launch shape of k_ed_verify.
#pragma once
#include "gvs_ed25519.h"

namespace gvs {
namespace sr {

constexpr int kXThreads = 256;             // 4 wavefronts
constexpr int kXItems = kXThreads / 4;     // 64 scalar multiplications per workgroup

GVS_SR_FN Fe fe_a24() { return fe_k(121665u, 0, 0, 0, 0, 0, 0, 0); }

// DPP quad_perm control: lane i of every quad reads lane s_i of its quad
__host__ __device__ constexpr int quad_perm(int s0, int s1, int s2, int s3) {
  return s0 | s1 << 2 | s2 << 4 | s3 << 6;
}

// ------------------------------------------------------------ the two quads
//
// The ladder below is written once over a quad type Q: V is "one field
// element in each of the four lanes", perm moves elements between lanes,
// pick<M> takes a where bit (lane) of M is set and b elsewhere, sel takes a
// where the quad's mask m is all ones.  QuadDev is one lane's view on the
// device (V is that lane's element); QuadHost is the four lanes in an array,
// every operation a loop over them, so the CPU build runs the same schedule.

struct QuadDev {
  using V = Fe;
  uint32_t lane;  // threadIdx.x & 3
  template <int P>
  GVS_SR_FN V perm(const V& x) const {
    V r = x;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int i = 0; i < 8; ++i)
      r.v[i] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x.v[i], P, 0xF, 0xF, false);
#endif
    return r;
  }
  template <int M>
  GVS_SR_FN V pick(const V& a, const V& b) const {
    return fe_select(0u - (((uint32_t)M >> lane) & 1u), a, b);
  }
  GVS_SR_FN V sel(uint32_t m, const V& a, const V& b) const { return fe_select(m, a, b); }
  GVS_SR_FN V splat(const Fe& c) const { return c; }
  GVS_SR_FN V add(const V& a, const V& b) const { return fe_add(a, b); }
  GVS_SR_FN V sub(const V& a, const V& b) const { return fe_sub(a, b); }
  GVS_SR_FN V mul(const V& a, const V& b) const { return fe_mul(a, b); }
  GVS_SR_FN V inv(const V& a) const { return fe_invert(a); }
  GVS_SR_FN V canon(const V& a) const { return fe_canon(a); }
};

struct QuadHost {
  struct V {
    Fe l[4];
  };
  template <int P>
  V perm(const V& x) const {
    V r;
    for (int i = 0; i < 4; ++i) r.l[i] = x.l[(P >> (2 * i)) & 3];
    return r;
  }
  template <int M>
  V pick(const V& a, const V& b) const {
    V r;
    for (int i = 0; i < 4; ++i) r.l[i] = fe_select(0u - (((uint32_t)M >> i) & 1u), a.l[i], b.l[i]);
    return r;
  }
  V sel(uint32_t m, const V& a, const V& b) const {
    V r;
    for (int i = 0; i < 4; ++i) r.l[i] = fe_select(m, a.l[i], b.l[i]);
    return r;
  }
  V splat(const Fe& c) const { return V{{c, c, c, c}}; }
#define GVS_X_LANES(name, expr)         \
  V name(const V& a, const V& b) const { \
    V r;                                 \
    for (int i = 0; i < 4; ++i) r.l[i] = expr(a.l[i], b.l[i]); \
    return r;                            \
  }
  GVS_X_LANES(add, fe_add)
  GVS_X_LANES(sub, fe_sub)
  GVS_X_LANES(mul, fe_mul)
#undef GVS_X_LANES
  V inv(const V& a) const { return V{{fe_invert(a.l[0]), fe_invert(a.l[1]), fe_invert(a.l[2]), fe_invert(a.l[3])}}; }
  V canon(const V& a) const { return V{{fe_canon(a.l[0]), fe_canon(a.l[1]), fe_canon(a.l[2]), fe_canon(a.l[3])}}; }
};

// ---------------------------------------------------------------- the ladder

// One step of RFC 7748 §5's ladder.  w = [X3 Z3 X2 Z2] in lanes 0..3; sw all
// ones to swap (2, 3) before the step.  Three multiply rounds.
template <class Q>
GVS_SR_FN typename Q::V x_step(const Q& q, const typename Q::V& w, const typename Q::V& x1, uint32_t sw) {
  using V = typename Q::V;
  // the conditional swap is the choice between w and its rotation by two lanes
  const V s = q.sel(sw, w, q.template perm<quad_perm(2, 3, 0, 1)>(w));    // [X2 Z2 X3 Z3]
  const V p = q.template perm<quad_perm(1, 0, 3, 2)>(s);                  // [Z2 X2 Z3 X3]
  const V sum = q.add(s, p);                                              // [A . C .]
  const V dif = q.sub(q.template pick<0xA>(p, s), q.template pick<0xA>(s, p));  // [. B . D]
  const V v = q.template pick<0xA>(dif, sum);                             // [A B C D]
  const V r1 = q.mul(q.template perm<quad_perm(0, 1, 0, 1)>(v),           // [A B A B]
                     q.template perm<quad_perm(3, 2, 0, 1)>(v));          // [D C A B] -> [DA CB AA BB]
  const V t = q.template perm<quad_perm(1, 0, 3, 2)>(r1);                 // [CB DA BB AA]
  const V s2 = q.add(r1, t);                                              // [DA+CB . . .]
  const V d2 = q.sub(t, r1);                                              // [. DA-CB . E]
  const V a2 = q.template pick<0x1>(s2, q.template pick<0x4>(r1, d2));    // [DA+CB DA-CB AA E]
  const V b2 = q.template pick<0x1>(s2, q.template pick<0x4>(t, q.template pick<0x8>(q.splat(fe_a24()), d2)));
  const V r2 = q.mul(a2, b2);                                             // [X3' (DA-CB)^2 X2' a24*E]
  const V a3 = q.template pick<0x8>(d2, r2);                              // [. (DA-CB)^2 . E]
  const V b3 = q.template pick<0x8>(q.add(t, r2), x1);                    // [. x1 . AA+a24*E]
  const V r3 = q.mul(a3, b3);                                             // [. Z3' . Z2'] (lanes 0, 2 dry)
  return q.template pick<0xA>(r3, r2);                                    // [X3' Z3' X2' Z2']
}

// decodeScalar25519 (RFC 7748 §5)
GVS_SR_FN Fe x_clamp(Fe k) {
  k.v[0] &= ~7u;
  k.v[7] = (k.v[7] & 0x7FFFFFFFu) | 0x40000000u;
  return k;
}

// X25519 of the (unclamped) scalar k and the u-coordinate u (the top bit
// ignored, u >= p reduced): the canonical result in every lane of the quad.
template <class Q>
GVS_SR_FN_NI typename Q::V x_ladder(const Q& q, Fe k, Fe u) {
  using V = typename Q::V;
  k = x_clamp(k);
  u.v[7] &= 0x7FFFFFFFu;
  const V x1 = q.splat(u);
  V w = q.template pick<0x1>(x1, q.template pick<0x8>(q.splat(fe_zero()), q.splat(fe_one())));  // [x1 1 1 0]
  uint32_t prev = 0;
#pragma unroll 1
  for (int i = 0; i < 255; ++i) {  // bits 254 .. 0: the scalar moves up under a fixed read position
#pragma unroll
    for (int j = 7; j > 0; --j) k.v[j] = (k.v[j] << 1) | (k.v[j - 1] >> 31);
    k.v[0] <<= 1;
    const uint32_t bit = 0u - (k.v[7] >> 31);
    w = x_step(q, w, x1, prev ^ bit);
    prev = bit;
  }
  const V s = q.sel(prev, w, q.template perm<quad_perm(2, 3, 0, 1)>(w));  // [X2 Z2 X3 Z3]
  const V x = q.template perm<quad_perm(0, 0, 0, 0)>(s), z = q.template perm<quad_perm(1, 1, 1, 1)>(s);
  return q.canon(q.mul(x, q.inv(z)));  // z = 0 gives 0
}

GVS_SR_FN Fe x_load(const uint8_t* p) {
  Fe r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = ld_le32(p + 4 * i);
  return r;
}

// Host form (tests/x25519_host.cpp): the four lanes' results; point null for
// the base point.
inline void x25519_quad_host(const uint8_t* scalar, const uint8_t* point, Fe out[4]) {
  const QuadHost::V r = x_ladder(QuadHost{}, x_load(scalar), point ? x_load(point) : fe_k(9, 0, 0, 0, 0, 0, 0, 0));
  for (int i = 0; i < 4; ++i) out[i] = r.l[i];
}

struct XArgs {
  const uint8_t* scalars;  // n 32-B scalars, scalar_stride bytes apart
  uint32_t scalar_stride;
  const uint8_t* points;   // n 32-B u-coordinates, point_stride apart; null: u = 9 for all
  uint32_t point_stride, n;
  uint8_t* out;            // n 32-B results, out_stride apart
  uint32_t out_stride;
  uint32_t* ok;            // n: 1 result non-zero, 0 all-zero (may be null)
};

__global__ void __launch_bounds__(kXThreads) k_x25519(XArgs a) {
  const uint32_t lane = threadIdx.x & 3u;
  const uint32_t k = blockIdx.x * kXItems + (threadIdx.x >> 2);
  const uint32_t kk = k < a.n ? k : a.n - 1;  // tail quads redo the last item: every lane stays in the DPP moves
  const Fe sc = x_load(a.scalars + (uint64_t)kk * a.scalar_stride);
  Fe u = fe_k(9, 0, 0, 0, 0, 0, 0, 0);
  if (a.points) u = x_load(a.points + (uint64_t)kk * a.point_stride);
  const Fe r = x_ladder(QuadDev{lane}, sc, u);
  if (k >= a.n) return;
  // lane j stores bytes [8j, 8j + 8): its two words by lane masks, not by index
  const uint32_t m0 = 0u - (uint32_t)(lane == 0), m1 = 0u - (uint32_t)(lane == 1),
                 m2 = 0u - (uint32_t)(lane == 2), m3 = 0u - (uint32_t)(lane == 3);
  const uint32_t lo = (r.v[0] & m0) | (r.v[2] & m1) | (r.v[4] & m2) | (r.v[6] & m3);
  const uint32_t hi = (r.v[1] & m0) | (r.v[3] & m1) | (r.v[5] & m2) | (r.v[7] & m3);
  uint8_t* o = a.out + (uint64_t)k * a.out_stride + 8u * lane;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    o[i] = (uint8_t)(lo >> (8 * i));
    o[4 + i] = (uint8_t)(hi >> (8 * i));
  }
  uint32_t any = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) any |= r.v[i];
  if (a.ok && lane == 0) a.ok[k] = any ? 1u : 0u;  // x25519-dalek's was_contributory
}

// ------------------------------------------------------- Noise HKDF-SHA-512

GVS_SR_FN uint64_t ld_be64(const uint8_t* p) {
  uint64_t x = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) x = (x << 8) | p[j];
  return x;
}

GVS_SR_FN void st_be64(uint8_t* p, uint64_t x) {
#pragma unroll
  for (int j = 0; j < 8; ++j) p[j] = (uint8_t)(x >> (56 - 8 * j));
}

// One item: ck 64 B, ikm ikm_len (0 or 32) B -> o1, o2 64 B each.  Twelve
// compressions in one rolled loop; c / 4 is the HMAC (temp, o1, o2), c % 4 its
// stage (key ^ ipad, message, key ^ opad, inner digest).  Keys, digests and
// outputs stay big-endian 64-bit words throughout: an HMAC's result is the
// next one's key as it stands.  Every branch is on c or ikm_len.
GVS_SR_FN_NI void noise_hkdf_one(const uint8_t* ck, const uint8_t* ikm, uint32_t ikm_len, uint8_t* o1,
                                 uint8_t* o2) {
  constexpr uint64_t kIv[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull,
                               0xa54ff53a5f1d36f1ull, 0x510e527fade682d1ull, 0x9b05688c2b3e6c1full,
                               0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
  constexpr uint64_t kIpad = 0x3636363636363636ull, kOpad = 0x5c5c5c5c5c5c5c5cull, kEnd = 0x80ull << 56;
  uint64_t key[8], m[4], h[8], inner[8], out1[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) key[i] = ld_be64(ck + 8 * i), h[i] = 0, inner[i] = 0, out1[i] = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) m[i] = ikm_len ? ld_be64(ikm + 8 * i) : 0;
#pragma unroll 1
  for (int c = 0; c < 12; ++c) {
    const int stage = c & 3, mac = c >> 2;
    uint64_t w[16], s[8];
    if (stage == 0 || stage == 2) {  // the padded key block, from the initial state
      const uint64_t pad = stage == 0 ? kIpad : kOpad;
#pragma unroll
      for (int i = 0; i < 8; ++i) w[i] = key[i] ^ pad, w[8 + i] = pad, h[i] = kIv[i];
    } else if (stage == 3) {  // the inner digest, 128 + 64 bytes hashed
#pragma unroll
      for (int i = 0; i < 8; ++i) w[i] = inner[i], w[8 + i] = 0;
      w[8] = kEnd;
      w[15] = 192u * 8u;
    } else {  // the message: ikm | 0x01 | o1 || 0x02
#pragma unroll
      for (int i = 0; i < 16; ++i) w[i] = 0;
      if (mac == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = m[i];
        w[0] = ikm_len ? w[0] : kEnd;
        w[4] = ikm_len ? kEnd : 0;
        w[15] = (128u + ikm_len) * 8u;
      } else if (mac == 1) {
        w[0] = 0x0180ull << 48;
        w[15] = 129u * 8u;
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) w[i] = out1[i];
        w[8] = 0x0280ull << 48;
        w[15] = 193u * 8u;
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] = h[i];
    sha512_rounds<0>(s, w);
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] += s[i];
    if (stage == 1) {
#pragma unroll
      for (int i = 0; i < 8; ++i) inner[i] = h[i];
    }
    if (stage == 3) {  // an HMAC is done: temp is the next key, o1 is kept, o2 ends
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        key[i] = mac == 0 ? h[i] : key[i];
        out1[i] = mac == 1 ? h[i] : out1[i];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    st_be64(o1 + 8 * i, out1[i]);
    st_be64(o2 + 8 * i, h[i]);
  }
}

struct HkdfArgs {
  const uint8_t* cks;  // n 64-B chaining keys, ck_stride apart
  uint32_t ck_stride;
  const uint8_t* ikm;  // n inputs of ikm_len bytes, ikm_stride apart (unused when ikm_len = 0)
  uint32_t ikm_stride, ikm_len, n;
  uint8_t *out1, *out2;  // n 64-B outputs each, out_stride apart
  uint32_t out_stride;
};

__global__ void __launch_bounds__(kSrThreads) k_noise_hkdf(HkdfArgs a) {
  const uint32_t k = blockIdx.x * kSrThreads + threadIdx.x;
  if (k >= a.n) return;
  noise_hkdf_one(a.cks + (uint64_t)k * a.ck_stride, a.ikm + (uint64_t)k * a.ikm_stride, a.ikm_len,
                 a.out1 + (uint64_t)k * a.out_stride, a.out2 + (uint64_t)k * a.out_stride);
}

}  // namespace sr
}  // namespace gvs
