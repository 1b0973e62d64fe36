// Host build of csrc/narrow.h (the 24-bit copy of a level-0 inverse): round
// trip, non-finite records and the byte offsets.  Built with
// -fsanitize=address,undefined by tests/test_narrow_format.py.
#define __host__
#define __device__
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "narrow.h"

using namespace mas;

static int fails = 0;
#define CHECK(c, ...)                     \
    do {                                  \
        if (!(c)) {                       \
            ++fails;                      \
            std::printf("FAIL %s: ", #c); \
            std::printf(__VA_ARGS__);     \
            std::printf("\n");            \
        }                                 \
    } while (0)

// Round trip of one record.  The bound is on the dequantised value q * s
// taken exactly (fp64 holds the 24 x 24-bit product): |q s - x| <= s / 2 =
// 2^-24 m (1 + 2^-23), m the record's largest magnitude; `slack` is 0 except
// where s is subnormal (its fp32 rounding is then absolute: 2^-149).  The
// fp32 decode must be that product correctly rounded, nothing else.
static double round_trip(const char* name, const float (&x)[kRecord], double slack = 0.0) {
    uint32_t w[kNarrowDwords];
    float s, y[kRecord];
    narrow_encode_record(x, w, s);
    narrow_decode_record(w, s, y);
    double m = 0.0;
    for (float v : x) m = std::fmax(m, std::fabs((double)v));
    const double bound = std::ldexp(m, -24) * (1.0 + std::ldexp(1.0, -23)) + slack;
    double worst = 0.0;
    for (int t = 0; t < kRecord / 4; ++t) {
        int q[4];
        narrow_unpack4(w[3 * t], w[3 * t + 1], w[3 * t + 2], q);
        for (int c = 0; c < 4; ++c) {
            const int f = 4 * t + c;
            const double exact = (double)q[c] * (double)s;
            const double e = std::fabs(exact - (double)x[f]);
            worst = std::fmax(worst, e);
            CHECK(q[c] >= -kNarrowQMax && q[c] <= kNarrowQMax, "%s entry %d q %d", name, f, q[c]);
            CHECK(e <= bound, "%s entry %d: x %.9g -> %.9g, error %.3g > bound %.3g", name, f, x[f], exact, e, bound);
            CHECK(y[f] == (float)exact, "%s entry %d: decode %.9g is not fl32(q s) %.9g", name, f, y[f], (float)exact);
        }
    }
    std::printf("%-28s m %.6g  s %.6g  worst |q s - x| %.4g  bound %.4g  (%.3f of it)\n", name, m, (double)s, worst,
                bound, bound > 0 ? worst / bound : 0.0);
    return worst;
}

static uint32_t rng_state = 12345u;
static float rnd() {  // in (-1, 1)
    rng_state = rng_state * 1664525u + 1013904223u;
    return (float)((int32_t)rng_state) * (1.0f / 2147483648.0f);
}

int main() {
    float x[kRecord];
    const float scales[] = {1.0f, 3.7e-6f, 8.1e5f, 1.0e-30f, 2.5e30f};
    for (float sc : scales) {
        // +-max and 0
        for (int f = 0; f < kRecord; ++f) x[f] = sc * rnd();
        x[0] = sc * 1.25f; x[1] = -sc * 1.25f; x[2] = 0.f; x[3] = -0.f;
        round_trip("random, +-max, 0", x);
        // one dominant entry
        for (int f = 0; f < kRecord; ++f) x[f] = sc * 1e-5f * rnd();
        x[37] = -sc * 3.0f;
        round_trip("one dominant entry", x);
        // all equal
        for (int f = 0; f < kRecord; ++f) x[f] = sc * 0.7f;
        round_trip("all equal", x);
        for (int f = 0; f < kRecord; ++f) x[f] = (f & 1) ? sc * 0.3f : -sc * 0.3f;
        round_trip("all equal magnitude", x);
    }
    // subnormal entries beside normal ones: they quantise to 0 within the bound
    for (int f = 0; f < kRecord; ++f) x[f] = (f % 3 ? 1.0f : -1.0f) * std::ldexp(1.0f, -140 + f % 13);
    x[11] = 0.5f;
    round_trip("subnormals beside 0.5", x);
    // a record of subnormals only (s itself is subnormal: absolute rounding)
    for (int f = 0; f < kRecord; ++f) x[f] = rnd() * std::ldexp(1.0f, -128);
    round_trip("subnormals only", x, std::ldexp(1.0, -149));
    for (int f = 0; f < kRecord; ++f) x[f] = 0.f;
    x[5] = std::numeric_limits<float>::denorm_min();
    round_trip("smallest subnormal", x, std::ldexp(1.0, -149));
    // the largest entry just above a rounded-down subnormal scale must not clamp
    for (int f = 0; f < kRecord; ++f) x[f] = 0.f;
    x[9] = 1.4999f * (float)kNarrowQMax * std::numeric_limits<float>::denorm_min();
    round_trip("subnormal scale, no clamp", x, std::ldexp(1.0, -149));
    // all zero: s = 0, q = 0, exact zeros (no 0/0)
    {
        for (int f = 0; f < kRecord; ++f) x[f] = (f & 1) ? 0.f : -0.f;
        uint32_t w[kNarrowDwords];
        float s, y[kRecord];
        narrow_encode_record(x, w, s);
        narrow_decode_record(w, s, y);
        CHECK(s == 0.f, "all-zero record: s %.9g", s);
        for (int d = 0; d < kNarrowDwords; ++d) CHECK(w[d] == 0u, "all-zero record: dword %d = %08x", d, w[d]);
        for (int f = 0; f < kRecord; ++f) CHECK(y[f] == 0.f, "all-zero record: entry %d decodes to %.9g", f, y[f]);
    }
    // non-finite: every entry of the record decodes to a non-finite value
    const float bads[] = {std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(),
                          std::numeric_limits<float>::quiet_NaN()};
    for (float bad : bads)
        for (int at : {0, 35, 71}) {
            for (int f = 0; f < kRecord; ++f) x[f] = rnd();
            x[(at + 7) % kRecord] = 0.f;
            x[at] = bad;
            uint32_t w[kNarrowDwords];
            float s, y[kRecord];
            narrow_encode_record(x, w, s);
            narrow_decode_record(w, s, y);
            for (int f = 0; f < kRecord; ++f) CHECK(!std::isfinite(y[f]), "bad %g at %d: entry %d = %.9g", bad, at, f, y[f]);
        }
    // pack / unpack over the extremes
    {
        const int q[4] = {kNarrowQMax, -kNarrowQMax, -1, 1};
        uint32_t w[3];
        int back[4];
        narrow_pack4(q, w);
        narrow_unpack4(w[0], w[1], w[2], back);
        for (int c = 0; c < 4; ++c) CHECK(back[c] == q[c], "pack4 %d: %d -> %d", c, q[c], back[c]);
    }
    // offsets: every slot's bytes distinct and in range, the scales and the
    // dword groups where the header says, 16-byte aligned per dword group
    {
        std::vector<int> owner(kNarrowBlockBytes, -1);
        auto claim = [&](int byte, int who) {
            CHECK(byte >= 0 && byte < kNarrowBlockBytes, "owner %d: byte %d out of range", who, byte);
            if (byte < 0 || byte >= kNarrowBlockBytes) return;
            CHECK(owner[byte] == -1, "byte %d claimed by %d and %d", byte, owner[byte], who);
            owner[byte] = who;
        };
        const int nSlots = kMainFloats + 48;
        for (int o = 0; o < nSlots; ++o)
            for (int k = 0; k < (o < kMainFloats ? 3 : 4); ++k) claim(narrow_slot_byte(o, k), o);
        for (int L = 0; L < 64; ++L)
            for (int k = 0; k < 4; ++k) claim(narrow_scale_off(L) + k, nSlots + L);
        int unowned = 0;
        for (int b : owner) unowned += b == -1;
        CHECK(unowned == 0, "%d bytes of a narrow block belong to no slot", unowned);
        CHECK(kNarrowBlockBytes == 14272 && kNarrowBlockBytes % 16 == 0 && kNarrowBlockBytes <= 14336, "block size %d",
              kNarrowBlockBytes);
        for (int L = 0; L < 64; ++L) {
            for (int g = 0; g < kNarrowGroups; ++g) {
                CHECK(narrow_dword_off(L, 4 * g) % 16 == 0, "lane %d group %d at %d", L, g, narrow_dword_off(L, 4 * g));
                CHECK(narrow_dword_off(L, 4 * g) == (g * 64 + L) * 16, "lane %d group %d", L, g);
                for (int c = 1; c < 4; ++c)
                    CHECK(narrow_dword_off(L, 4 * g + c) == narrow_dword_off(L, 4 * g) + 4 * c, "lane %d group %d", L, g);
            }
            CHECK(narrow_dword_off(L, 52) % 8 == 0 && narrow_dword_off(L, 53) == narrow_dword_off(L, 52) + 4,
                  "lane %d last group", L);
        }
        CHECK(kNarrowLastOff % 16 == 0 && kNarrowScaleOff % 16 == 0 && kNarrowTailOff % 16 == 0, "piece offsets");
        // a slot's three bytes are entry f of its lane's little-endian stream
        for (int o = 0; o < kMainFloats; ++o) {
            const int F = o >> 2, L = F & 63, f = 4 * (F >> 6) + (o & 3);
            for (int k = 0; k < 3; ++k) {
                const int p = 3 * f + k;
                CHECK(narrow_slot_byte(o, k) == narrow_dword_off(L, p >> 2) + (p & 3), "slot %d byte %d", o, k);
            }
        }
    }
    if (fails) {
        std::printf("%d check(s) failed\n", fails);
        return 1;
    }
    std::printf("narrow format ok\n");
    return 0;
}
