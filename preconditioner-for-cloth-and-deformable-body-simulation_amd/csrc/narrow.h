// narrow.h -- the 24-bit copy of one level-0 packed inverse that the fine
// apply kernel streams (k_apply.hip; written by k_narrow_inv, k_factor.hip).
//
// A narrow block holds the same 4656 slots as a packed fp32 block (layout.h),
// in the same lane and record order: lane L's record is still its 72 entries
// f = 0..71, and the tail is still row 2 of G(p, p+16).  Only the storage of
// a record changes: every entry is a signed 24-bit integer q, and the record
// carries one fp32 scale s,
//
//   m = max |x| over the record,  s = fl32(m / 8388607),
//   q = rint(x / s) clamped to +-8388607,          decode  x' = float(q) * s
//
// so |x' - x| <= s / 2 = 2^-24 m (1 + 2^-23) before the decode's own fp32
// rounding.  (q is formed in fp64, x * (1 / s): an fp32 quotient near 2^23
// has an ulp of 1/2 and could round to the wrong neighbour.  Where s is
// subnormal its fp32 rounding is absolute, not relative; it is then stepped
// up once if m / s would otherwise clamp, which adds at most 2^-150 to the
// bound.)  An all-zero record has s = 0, q = 0 and decodes to exact zeros; a
// record with a non-finite entry has s = NaN and decodes to NaN throughout,
// so a failed block shows in z as it does with the fp32 inverses.
//
// The 72 q of a record are a little-endian stream of 216 bytes = 54 dwords
// (entry f = bytes 3f .. 3f+2), loaded as 13 dwordx4 and one dwordx2:
//
//   bytes      0 .. 13 311   dword group g = 0..12 of lane L (dwords 4g..4g+3)
//                            at uint4 index g*64 + L
//         13 312 .. 13 823   dwords 52, 53 of lane L at uint2 index L
//         13 824 .. 14 079   scale of lane L at float index L
//         14 080 .. 14 271   the 48-float tail, fp32 as in layout.h
//
// 14 272 B per block (a multiple of 16) against 18 624 B; every wave load of
// the main part still reads 1 KiB contiguous (512 B for the last group).
#pragma once

#include <cstdint>

#include "layout.h"

namespace mas {

constexpr int kNarrowQMax = 8388607;          // 2^23 - 1
constexpr int kNarrowDwords = 54;             // per lane record: 72 * 3 bytes
constexpr int kNarrowGroups = 13;             // full dwordx4 groups per lane
constexpr int kNarrowLastOff = kNarrowGroups * 64 * 16;   // 13 312: the dwordx2 group
constexpr int kNarrowScaleOff = kNarrowLastOff + 64 * 8;  // 13 824
constexpr int kNarrowTailOff = kNarrowScaleOff + 64 * 4;  // 14 080
constexpr int kNarrowBlockBytes = kNarrowTailOff + 48 * 4;  // 14 272

// byte offset, inside a narrow block, of dword d (0..53) of lane L's record
__host__ __device__ inline int narrow_dword_off(int L, int d) {
    const int g = d >> 2, c = d & 3;
    return g < kNarrowGroups ? (g * 64 + L) * 16 + c * 4 : kNarrowLastOff + L * 8 + c * 4;
}

// byte offset of byte k of packed slot o (layout.h's float offset): k = 0..2
// for a main-part slot (least significant first), 0..3 for a tail slot
__host__ __device__ inline int narrow_slot_byte(int o, int k) {
    if (o >= kMainFloats) return kNarrowTailOff + 4 * (o - kMainFloats) + k;
    const int F = o >> 2, L = F & 63, f = 4 * (F >> 6) + (o & 3);
    const int p = 3 * f + k;
    return narrow_dword_off(L, p >> 2) + (p & 3);
}

__host__ __device__ inline int narrow_scale_off(int L) { return kNarrowScaleOff + 4 * L; }

// the record's scale from its largest magnitude m (bad: it holds a non-finite entry)
__host__ __device__ inline float narrow_scale(float m, bool bad) {
    if (bad) return __builtin_nanf("");
    if (m == 0.f) return 0.f;
    float s = m / (float)kNarrowQMax;
    // a subnormal s was rounded absolutely: never let the largest entry clamp
    if ((double)s * ((double)kNarrowQMax + 0.5) <= (double)m)
        s = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, s) + 1u);
    return s;
}

// q of entry x under scale s; rs = 1 / (double)s (unused where s is 0 or NaN)
__host__ __device__ inline int narrow_quant(float x, float s, double rs) {
    if (!(s > 0.f)) return 0;
    double t = __builtin_rint((double)x * rs);
    t = t > (double)kNarrowQMax ? (double)kNarrowQMax : t;
    t = t < -(double)kNarrowQMax ? -(double)kNarrowQMax : t;
    return (int)t;
}

__host__ __device__ inline float narrow_decode(int q, float s) { return (float)q * s; }

// four q <-> three dwords (a 12-byte little-endian run of the record's stream)
__host__ __device__ inline void narrow_pack4(const int (&q)[4], uint32_t (&w)[3]) {
    const uint32_t a = (uint32_t)q[0] & 0xffffffu, b = (uint32_t)q[1] & 0xffffffu;
    const uint32_t c = (uint32_t)q[2] & 0xffffffu, d = (uint32_t)q[3] & 0xffffffu;
    w[0] = a | (b << 24);
    w[1] = (b >> 8) | (c << 16);
    w[2] = (c >> 16) | (d << 8);
}

__host__ __device__ inline void narrow_unpack4(uint32_t w0, uint32_t w1, uint32_t w2, int (&q)[4]) {
    q[0] = (int32_t)(w0 << 8) >> 8;
    q[1] = (int32_t)(((w0 >> 24) | (w1 << 8)) << 8) >> 8;
    q[2] = (int32_t)(((w1 >> 16) | (w2 << 16)) << 8) >> 8;
    q[3] = (int32_t)w2 >> 8;
}

// one record: 72 fp32 entries -> its scale and 54 dwords
__host__ __device__ inline void narrow_encode_record(const float (&x)[kRecord], uint32_t (&w)[kNarrowDwords],
                                                     float& s) {
    float m = 0.f;
    bool bad = false;
    for (int f = 0; f < kRecord; ++f) {
        const float a = __builtin_fabsf(x[f]);
        bad |= !(a <= 3.402823466e+38f);  // inf or NaN
        m = a > m ? a : m;
    }
    s = narrow_scale(m, bad);
    const double rs = s > 0.f ? 1.0 / (double)s : 0.0;
    for (int t = 0; t < kRecord / 4; ++t) {
        int q[4];
        uint32_t o[3];
        for (int c = 0; c < 4; ++c) q[c] = narrow_quant(x[4 * t + c], s, rs);
        narrow_pack4(q, o);
        w[3 * t + 0] = o[0];
        w[3 * t + 1] = o[1];
        w[3 * t + 2] = o[2];
    }
}

__host__ __device__ inline void narrow_decode_record(const uint32_t (&w)[kNarrowDwords], float s,
                                                     float (&x)[kRecord]) {
    for (int t = 0; t < kRecord / 4; ++t) {
        int q[4];
        narrow_unpack4(w[3 * t], w[3 * t + 1], w[3 * t + 2], q);
        for (int c = 0; c < 4; ++c) x[4 * t + c] = narrow_decode(q[c], s);
    }
}

}  // namespace mas
