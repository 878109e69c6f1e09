// gvs_noise.h — the responder's side of Noise_IX_25519_AESGCM_SHA512 (Noise
// specification rev. 34, pattern IX: -> e, s   <- e, ee, se, s, es) on the
// device, batched over handshakes: k_noise_ix<PHASE> is the symmetric state
// (MixHash, MixKey, Split) between the launches of k_x25519 and k_aead<true>
// that gvs_noise_ix_respond chains.
//
// One DPP quad per handshake, k_x25519's launch shape.  The kernel is a
// compression schedule: a rolled loop of steps around one inlined copy of the
// SHA-512 rounds; in every step each lane of the quad runs one compression on
// its own (state, block) pair, and what it keeps of the result is a select on
// its lane number and the step number.
//   lane 0   HMAC inner: the key ^ ipad block, then the message block
//   lane 1   HMAC outer: the key ^ opad block, then the inner digest
//   lane 2   the transcript: the chain of h, one block of H(h | x) per step
//   lane 3   dry: it shadows lane 2 and stores nothing
// An HKDF is eight steps on lanes 0 and 1:
//   0  ck ^ ipad | ck ^ opad         4  0x01              (lane 0)
//   1  the message        (lane 0)   5  outer -> o1       (lane 1)
//   2  outer -> temp      (lane 1)   6  o1 | 0x02         (lane 0)
//   3  temp ^ ipad | temp ^ opad,    7  outer -> o2       (lane 1)
//      both states kept
// ten compressions, eight deep: o1 and o2 start from temp's two pad states.
// After every step the lanes of each pair (0, 1) and (2, 3) exchange their
// results by one quad_perm DPP move of the digest (16 moves of 32 bits), so the
// inner digest reaches lane 1 and temp, o1 and o2 reach lane 0.  No LDS, no
// ds_bpermute.  Digests, keys and blocks stay big-endian 64-bit words, as in
// noise_hkdf_one: an output is the next key or the next block as it stands.
//
// What depends on data: the transcript's block count follows the lengths the
// peer sent in clear (payload 1, per item) and the call's prologue and payload
// 2 lengths; a step whose block lies past an item's last one runs and is
// dropped by a select.  e, s, the DH outputs, ck and k reach no branch and no
// address.  An item that fails (a message 1 shorter than 64 or longer than 128
// bytes, an all-zero ee, se or es) runs every step; phase C zeroes what it
// would have returned.
//
// The schedule is written once over a quad type, like x_step: NxQuadDev is one
// lane's view on the device, NxQuadHost the four lane states stepped in a loop
// (tests/noise_host.cpp).
#pragma once
#include "gvs_x25519.h"

namespace gvs {
namespace sr {

constexpr uint32_t kNxPayload1Max = 64;  // GVS_NOISE_PAYLOAD1_MAX
constexpr uint32_t kNxPrologueMax = 64;  // GVS_NOISE_PROLOGUE_MAX
constexpr uint32_t kNxMsg2Fixed = 96;    // e_pub 32 | ct_s 48 | ct_p's tag 16
constexpr int kNxA = 0, kNxB = 1, kNxC = 2;

// blocks of H(h | x), x of len bytes: 64 + len + 0x80 + the 16-byte bit count
__host__ __device__ constexpr uint32_t nx_blocks(uint32_t len) { return (64u + len + 17u + 127u) >> 7; }
// phase C's trip count for a payload 2 of p2 bytes
__host__ __device__ constexpr uint32_t nx_steps_c(uint32_t p2) {
  return nx_blocks(p2 + 16u) > 8u ? nx_blocks(p2 + 16u) : 8u;
}

// One call's arrays.  x25519 item 4i + k of handshake i is e_pub (k = 0), ee,
// se, es; item 4n is s_pub.
struct NxArgs {
  uint32_t n, p2, steps_c;
  const uint8_t* msg1;       // re 32 | rs 32 | payload 1, msg1_stride (>= 64) apart
  uint32_t msg1_stride;
  const uint32_t* msg1_lens;
  const uint8_t* pro;        // the prologue in a 64-byte cell
  uint32_t pro_len;
  const uint8_t* xout;       // (4n + 1) x 32 B: k_x25519's results
  const uint32_t* xok;       // and their non-zero flags
  uint8_t* st;               // n x 128 B between the phases: ck 64 | h 64
  uint8_t* key;              // n x 32 B: the next k_aead's keys
  uint8_t* aad;              // n x 64 B: its AAD (h)
  uint8_t* text1;            // n x 32 B: s_pub, the first seal's text
  const uint8_t* ct1;        // n x 48 B: ct_s
  const uint8_t* ct2;        // ct_p, ct2_stride (>= p2 + 16) apart
  uint32_t ct2_stride;
  uint8_t* msg2;             // the caller's slots, msg2_stride (>= 96 + p2) apart, written whole
  uint32_t msg2_stride;
  uint32_t* msg2_lens;
  uint8_t *recv, *send;      // n x 32 B: k1, k2
  uint8_t* hashes;           // n x 64 B, may be null
  uint32_t* ok;
};

// one lane's registers
struct NxLane {
  uint64_t key[8];  // lanes 0, 1: the HMAC key (ck, temp), then o1; lanes 2, 3: h
  uint64_t hs[8];   // the running hash state
  uint64_t ps[8];   // lanes 0, 1: temp's pad state, then o2
  uint64_t mb[8];   // the pair partner's last result
  uint64_t r[8];    // this lane's last result
  uint64_t act, last;  // lanes 2, 3: the step's block exists for this item / is its last
};

struct NxQuadDev {
  uint32_t lane;  // threadIdx.x & 3
  NxLane L;
  template <class F>
  GVS_SR_FN void each(F f) { f(lane, L); }
  GVS_SR_FN void swap() {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)L.r[i], quad_perm(1, 0, 3, 2), 0xF, 0xF, false);
      const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(L.r[i] >> 32), quad_perm(1, 0, 3, 2), 0xF, 0xF, false);
      L.mb[i] = (uint64_t)hi << 32 | lo;
    }
#endif
  }
};

struct NxQuadHost {
  NxLane L[4];
  template <class F>
  void each(F f) {
    for (uint32_t l = 0; l < 4; ++l) f(l, L[l]);
  }
  void swap() {
    for (int l = 0; l < 4; ++l)
      for (int i = 0; i < 8; ++i) L[l].mb[i] = L[l ^ 1].r[i];
  }
};

GVS_SR_FN uint64_t nx_sel(uint64_t m, uint64_t a, uint64_t b) { return (a & m) | (b & ~m); }

// x of a MixHash: p[base .. base + len), p readable below cap
struct NxSeg {
  const uint8_t* p;
  uint32_t base, len, cap;
};

// the big-endian word at offset off of x | 0x80 | 0 ...; reads stay below cap
GVS_SR_FN uint64_t nx_xword(const NxSeg& s, uint32_t off) {
  uint64_t x = 0;
#pragma unroll
  for (uint32_t j = 0; j < 8; ++j) {
    const uint32_t pos = off + j, at = s.base + pos;
    const uint32_t b = s.p[at < s.cap ? at : s.cap - 1u];
    x = (x << 8) | (pos < s.len ? b : (pos == s.len ? 0x80u : 0u));
  }
  return x;
}

// The transcript's step table: what lanes 2 and 3 hash in step t of a phase,
// block b of H(h | s).  False: nothing (the step is dry for them).
template <int PH>
GVS_SR_FN bool nx_slot(const NxArgs& a, uint32_t i, uint32_t l1, int t, NxSeg& s, uint32_t& b) {
  const uint8_t* m1 = a.msg1 + (uint64_t)i * a.msg1_stride;
  b = 0;
  if (PH == kNxA) {
    if (t < 2) {  // the prologue: two slots
      s = NxSeg{a.pro, 0u, a.pro_len, kNxPrologueMax};
      b = (uint32_t)t;
    } else if (t == 2) {
      s = NxSeg{m1, 0u, 32u, 64u};  // re
    } else if (t == 3) {
      s = NxSeg{m1, 32u, 32u, 64u};  // rs
    } else if (t < 6) {  // payload 1: two slots, even when it is empty
      s = NxSeg{m1, 64u, l1, a.msg1_stride};
      b = (uint32_t)t - 4u;
    } else if (t == 6) {
      s = NxSeg{a.xout + 128u * (uint64_t)i, 0u, 32u, 32u};  // e_pub
    } else {
      return false;
    }
  } else if (PH == kNxB) {
    if (t >= 2) return false;
    s = NxSeg{a.ct1 + 48u * (uint64_t)i, 0u, 48u, 48u};  // ct_s: 112 bytes hashed, two blocks
    b = (uint32_t)t;
  } else {
    if ((uint32_t)t >= nx_blocks(a.p2 + 16u)) return false;
    s = NxSeg{a.ct2 + (uint64_t)i * a.ct2_stride, 0u, a.p2 + 16u, a.ct2_stride};  // ct_p
    b = (uint32_t)t;
  }
  return true;
}

constexpr uint64_t kNxIpad = 0x3636363636363636ull, kNxOpad = 0x5c5c5c5c5c5c5c5cull, kNxEnd = 0x80ull << 56;

// Step t, first half: the lane's block and input state, one compression, the
// result in L.r.  u is the HKDF's step on lanes 0 and 1 (-1: none left).
template <int PH>
GVS_SR_FN void nx_front(const NxArgs& a, uint32_t i, uint32_t l1, int t, uint32_t lane, NxLane& L) {
  constexpr uint64_t kIv[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull,
                               0xa54ff53a5f1d36f1ull, 0x510e527fade682d1ull, 0x9b05688c2b3e6c1full,
                               0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
  const int u = t < (PH == kNxA ? 16 : 8) ? (t & 7) : -1;
  const uint64_t tx = 0ull - (uint64_t)(lane >= 2u);
  uint64_t w[16], s[8];
#pragma unroll
  for (int j = 0; j < 16; ++j) w[j] = 0;
  bool fresh = false;
  if (u == 0 || u == 3) {  // the padded key block, from the initial state
    const uint64_t pad = lane == 0 ? kNxIpad : kNxOpad;
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = L.key[j] ^ pad, w[8 + j] = pad;
    fresh = true;
  } else if (u == 1) {  // the HKDF's input: a DH output, or nothing (Split)
    if (PH == kNxC) {
      w[0] = kNxEnd;
      w[15] = 128u * 8u;
    } else {
      const uint8_t* ikm = a.xout + 32u * (4u * (uint64_t)i + (PH == kNxA ? 1u + (uint32_t)(t >> 3) : 3u));
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = ld_be64(ikm + 8 * j);
      w[4] = kNxEnd;
      w[15] = 160u * 8u;
    }
  } else if (u == 4) {
    w[0] = 0x0180ull << 48;
    w[15] = 129u * 8u;
  } else if (u == 6) {
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = L.key[j];  // o1
    w[8] = 0x0280ull << 48;
    w[15] = 193u * 8u;
  } else if (u >= 0) {  // 2, 5, 7: the outer block over the partner's inner digest
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = L.mb[j];
    w[8] = kNxEnd;
    w[15] = 192u * 8u;
  }
  uint64_t fm = fresh ? ~tx : 0;  // lanes that start from the initial state
  NxSeg sg;
  uint32_t b;
  L.act = L.last = 0;
  if (nx_slot<PH>(a, i, l1, t, sg, b)) {
    const uint32_t nb = nx_blocks(sg.len);
    L.act = 0ull - (uint64_t)(b < nb);
    L.last = 0ull - (uint64_t)(b + 1u == nb);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      uint64_t x;
      if (b == 0 && j < 8)
        x = L.key[j];  // h
      else
        x = nx_xword(sg, 128u * b + 8u * (uint32_t)j - 64u);
      if (j == 15) x |= L.last & (uint64_t)(64u + sg.len) * 8u;
      w[j] = nx_sel(tx, x, w[j]);
    }
    if (b == 0) fm |= tx;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = L.r[j] = nx_sel(fm, kIv[j], L.hs[j]);
  sha512_rounds<0>(s, w);
#pragma unroll
  for (int j = 0; j < 8; ++j) L.r[j] += s[j];
}

// Step t, second half, after the pairs exchanged results: what each lane keeps
template <int PH>
GVS_SR_FN void nx_back(int t, uint32_t lane, NxLane& L) {
  const int u = t < (PH == kNxA ? 16 : 8) ? (t & 7) : -1;
  const uint64_t l0 = 0ull - (uint64_t)(lane == 0u), l1 = 0ull - (uint64_t)(lane == 1u), kk = l0 | l1;
  // lanes 0, 1
  const uint64_t keep_hs = (u == 0 || u == 3) ? kk : ((u == 1 || u == 4 || u == 6) ? l0 : 0);
  const uint64_t both = (u == 2 || u == 5 || u == 7) ? kk : 0;  // lane 1's result, on both lanes
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const uint64_t o = nx_sel(l1, L.r[j], L.mb[j]);
    L.hs[j] = nx_sel(keep_hs, L.r[j], L.hs[j]);
    if (u == 3) L.ps[j] = nx_sel(kk, L.r[j], L.ps[j]);
    if (u == 2 || u == 5) L.key[j] = nx_sel(both, o, L.key[j]);  // temp; o1, the next ck
    if (u == 5) L.hs[j] = nx_sel(kk, L.ps[j], L.hs[j]);           // o2 starts from temp's pad states too
    if (u == 7) L.ps[j] = nx_sel(both, o, L.ps[j]);               // o2
    // lanes 2, 3
    L.hs[j] = nx_sel(L.act & ~kk, L.r[j], L.hs[j]);
    L.key[j] = nx_sel(L.act & L.last & ~kk, L.r[j], L.key[j]);
  }
}

GVS_SR_FN void nx_st64(uint8_t* p, const uint64_t* v, int words, uint64_t mask) {
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (j < words) st_be64(p + 8 * j, v[j] & mask);
}

// What a phase leaves behind, a part per lane
template <int PH>
GVS_SR_FN void nx_store(const NxArgs& a, uint32_t i, bool len_ok, uint32_t lane, const NxLane& L) {
  const uint64_t all = ~0ull;
  if (PH != kNxC) {
    uint8_t* st = a.st + 128u * (uint64_t)i;
    if (lane == 0) nx_st64(st, L.key, 8, all);                       // ck
    if (lane == 1) nx_st64(a.key + 32u * (uint64_t)i, L.ps, 4, all);  // k = o2[0:32]
    if (lane == 2) {
      nx_st64(st + 64, L.key, 8, all);  // h, and h as the seal's AAD
      nx_st64(a.aad + 64u * (uint64_t)i, L.key, 8, all);
    }
    if (PH == kNxA && lane == 3) {
      const uint8_t* sp = a.xout + 128u * (uint64_t)a.n;  // s_pub
#pragma unroll
      for (int j = 0; j < 32; ++j) a.text1[32u * (uint64_t)i + j] = sp[j];
    }
    return;
  }
  const uint32_t* xk = a.xok + 4u * (uint64_t)i;
  const uint32_t good = (uint32_t)len_ok & (uint32_t)(xk[1] != 0) & (uint32_t)(xk[2] != 0) & (uint32_t)(xk[3] != 0);
  const uint64_t m = 0ull - (uint64_t)good;
  if (lane == 0) nx_st64(a.recv + 32u * (uint64_t)i, L.key, 4, m);  // k1 = o1[0:32]
  if (lane == 1) nx_st64(a.send + 32u * (uint64_t)i, L.ps, 4, m);   // k2 = o2[0:32]
  if (lane == 2 && a.hashes) nx_st64(a.hashes + 64u * (uint64_t)i, L.key, 8, m);
  if (lane == 3) {
    a.ok[i] = good;
    a.msg2_lens[i] = good ? kNxMsg2Fixed + a.p2 : 0u;
  }
  // message 2 = e_pub | ct_s | ct_p, the rest of the slot zero: byte j by lane j % 4
  const uint8_t *ep = a.xout + 128u * (uint64_t)i, *c1 = a.ct1 + 48u * (uint64_t)i,
                *c2 = a.ct2 + (uint64_t)i * a.ct2_stride;
  uint8_t* o = a.msg2 + (uint64_t)i * a.msg2_stride;
  const uint32_t end = kNxMsg2Fixed + a.p2;
  for (uint32_t j = lane; j < a.msg2_stride; j += 4u) {
    uint32_t v = 0;
    if (j < 32u)
      v = ep[j];
    else if (j < 80u)
      v = c1[j - 32u];
    else if (j < end)
      v = c2[j - 80u];
    o[j] = (uint8_t)(v & (uint32_t)m);
  }
}

// One handshake's phase: load, the schedule, store (live: not a tail quad's
// repeat of the last item)
// CHACHAPOLY: the suite's cipher, which only the protocol name of phase A sees
template <int PH, bool CHACHAPOLY = false, class Q>
GVS_SR_FN_NI void nx_item(Q& q, const NxArgs& a, uint32_t i, bool live) {
  const uint32_t len1 = a.msg1_lens[i];
  const bool len_ok = (len1 >= 64u) & (len1 <= 64u + kNxPayload1Max);
  const uint32_t l1 = len_ok ? len1 - 64u : 0u;
  q.each([&](uint32_t lane, NxLane& L) {
    // "Noise_IX_25519_AESGCM_SHA512" zero-padded to 64 bytes: h0, and ck = h0
    constexpr uint64_t kNameGcm[8] = {0x4e6f6973655f4958ull, 0x5f32353531395f41ull, 0x455347434d5f5348ull,
                                      0x4135313200000000ull, 0, 0, 0, 0};
    // "Noise_IX_25519_ChaChaPoly_SHA512": 32 bytes, padded the same way
    constexpr uint64_t kNameCp[8] = {0x4e6f6973655f4958ull, 0x5f32353531395f43ull, 0x6861436861506f6cull,
                                     0x795f534841353132ull, 0, 0, 0, 0};
    const uint8_t* st = a.st + 128u * (uint64_t)i + (lane >= 2u ? 64u : 0u);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      L.key[j] = PH == kNxA ? (CHACHAPOLY ? kNameCp[j] : kNameGcm[j]) : ld_be64(st + 8 * j);
      L.hs[j] = L.ps[j] = L.mb[j] = L.r[j] = 0;
    }
    L.act = L.last = 0;
  });
  const int steps = PH == kNxA ? 16 : (PH == kNxB ? 8 : (int)a.steps_c);
#pragma unroll 1
  for (int t = 0; t < steps; ++t) {
    q.each([&](uint32_t lane, NxLane& L) { nx_front<PH>(a, i, l1, t, lane, L); });
    q.swap();
    q.each([&](uint32_t lane, NxLane& L) { nx_back<PH>(t, lane, L); });
  }
  if (live) q.each([&](uint32_t lane, NxLane& L) { nx_store<PH>(a, i, len_ok, lane, L); });
}

// Host form (tests/noise_host.cpp): one handshake's phase on four lane states.
// False if the lanes disagree where they hold the same value: ck and o2 on
// lanes 0 and 1, h on lanes 2 and 3.
template <int PH>
inline bool nx_item_host(const NxArgs& a, uint32_t i) {
  NxQuadHost q;
  nx_item<PH>(q, a, i, true);
  uint64_t d = 0;
  for (int j = 0; j < 8; ++j)
    d |= (q.L[0].key[j] ^ q.L[1].key[j]) | (q.L[0].ps[j] ^ q.L[1].ps[j]) | (q.L[2].key[j] ^ q.L[3].key[j]);
  return d == 0;
}

#if defined(__HIPCC__)

template <int PH>
__global__ void __launch_bounds__(kXThreads) k_noise_ix(NxArgs a) {
  const uint32_t k = blockIdx.x * kXItems + (threadIdx.x >> 2);
  const uint32_t kk = k < a.n ? k : a.n - 1;  // tail quads redo the last item: every lane stays in the DPP moves
  NxQuadDev q;
  q.lane = threadIdx.x & 3u;
  nx_item<PH>(q, a, kk, k < a.n);
}

// Phase A of Noise_IX_25519_ChaChaPoly_SHA512: the same schedule from the
// other protocol name.  Phases B and C do not see the name.
__global__ void __launch_bounds__(kXThreads) k_noise_ix_a_chachapoly(NxArgs a) {
  const uint32_t k = blockIdx.x * kXItems + (threadIdx.x >> 2);
  const uint32_t kk = k < a.n ? k : a.n - 1;
  NxQuadDev q;
  q.lane = threadIdx.x & 3u;
  nx_item<kNxA, true>(q, a, kk, k < a.n);
}

// What the chain's first launches read, put where their fixed strides want
// it: k_x25519's 4n + 1 (scalar, point) rows, the prologue cell, the seals'
// nonces (Noise's counter 0: all zero) and lengths, and payload 2 as the
// second seal's 16-byte-strided text.
struct NxGatherArgs {
  uint8_t s[32];             // the responder's static secret
  uint8_t pro[64];           // the prologue, zero-padded
  const uint8_t* eph;        // n x 32 B
  const uint8_t* msg1;
  uint32_t msg1_stride;
  const uint8_t* payload;    // payload_stride apart (0: one for all); unused when p2 = 0
  uint32_t payload_stride, p2, text2_stride, n;
  uint8_t *xsc, *xpt;        // (4n + 1) x 32 B each
  uint8_t* pro_out;          // 64 B
  uint32_t* iv;              // n x 12 B
  uint32_t *aad_lens, *len1, *len2;
  uint8_t* text2;
};

__global__ void __launch_bounds__(kXThreads) k_noise_ix_gather(NxGatherArgs a) {
  const uint32_t i = blockIdx.x * kXItems + (threadIdx.x >> 2), k = threadIdx.x & 3u;
  if (i < a.n) {  // row 4i + k: (e, 9), (e, re), (e, rs), (s, re)
    const uint8_t* e = a.eph + 32u * (uint64_t)i;
    const uint8_t* pt = a.msg1 + (uint64_t)i * a.msg1_stride + (k == 2u ? 32u : 0u);
    uint8_t *sc = a.xsc + 32u * (4u * (uint64_t)i + k), *pp = a.xpt + 32u * (4u * (uint64_t)i + k);
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      const uint8_t ev = e[j], pv = pt[j];
      sc[j] = k == 3u ? a.s[j] : ev;
      pp[j] = k == 0u ? (uint8_t)(j == 0 ? 9 : 0) : pv;
    }
    if (k < 3u) a.iv[3u * (uint64_t)i + k] = 0;
    if (k == 0u) a.aad_lens[i] = 64u, a.len1[i] = 32u, a.len2[i] = a.p2;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {  // row 4n: (s, 9), and the prologue cell
    uint8_t *sc = a.xsc + 128u * (uint64_t)a.n, *pp = a.xpt + 128u * (uint64_t)a.n;
#pragma unroll
    for (int j = 0; j < 32; ++j) sc[j] = a.s[j], pp[j] = (uint8_t)(j == 0 ? 9 : 0);
#pragma unroll
    for (int j = 0; j < 64; ++j) a.pro_out[j] = a.pro[j];
  }
  // the workgroup's 64 payloads, byte after byte across its threads
  const uint32_t i0 = blockIdx.x * kXItems;
  for (uint32_t x = threadIdx.x; x < kXItems * a.text2_stride; x += kXThreads) {
    const uint32_t it = i0 + x / a.text2_stride, off = x % a.text2_stride;
    if (it >= a.n) break;
    a.text2[(uint64_t)it * a.text2_stride + off] =
        off < a.p2 ? a.payload[(uint64_t)it * a.payload_stride + off] : (uint8_t)0;
  }
}

#endif  // __HIPCC__

}  // namespace sr
}  // namespace gvs
