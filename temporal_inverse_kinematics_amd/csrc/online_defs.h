// online_defs.h — what the dataflow kernel (online.hip) and the plain C++ that
// plans its step (stream_plan.h) both read, from one definition and with no HIP
// include: the kernel's limits, the phase and residual kinds, the phase record,
// and the fp32 <-> bf16 helpers of every bf16x3 weight pack (common.h).
#pragma once
#include <cstring>

namespace tik {

constexpr int ONL_MAXL = 12;        // layers
constexpr int ONL_MAXC = 256;       // channels per layer
constexpr int ONL_MAXHC = 17;       // head K chunks of 4 per lane: K <= 17 * 4 * 64 = 4352 = 17 joints x ONL_MAXC
constexpr int ONL_MAXPH = 2 * ONL_MAXL + 3;   // phases: G and T per layer, the head
enum { ONP_G = 1, ONP_T = 2, ONP_H = 3 };
enum { ONR_ZERO = 0, ONR_IDEN = 1, ONR_CONV = 2 };

struct OnlinePhase {
    int kind, layer, nframes, ngroups, task0, cbase;   // cbase: the phase's counter (the head's: tasks done)
};

}  // namespace tik

namespace tik_host {

// fp32 -> bf16 bits, round to nearest even (finite inputs; NaN stays NaN)
inline unsigned short bf16_rne(float x) {
    unsigned u;
    memcpy(&u, &x, 4);
    if ((u & 0x7f800000u) == 0x7f800000u) return (unsigned short)((u >> 16) | ((u & 0xffffu) ? 0x40u : 0u));
    return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
inline float bf16_to_f32(unsigned short b) {
    const unsigned u = (unsigned)b << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
// x = p0 + p1 + p2 with p_i = bf16_rne(x - p0 - ... - p_{i-1}): exact for
// normal fp32 x (each plane takes the next 8 significant bits, the
// residuals are exact in fp32), full fp32 exponent range
inline void split_bf16x3(float x, unsigned short& p0, unsigned short& p1, unsigned short& p2) {
    p0 = bf16_rne(x);
    const float r1 = x - bf16_to_f32(p0);
    p1 = bf16_rne(r1);
    const float r2 = r1 - bf16_to_f32(p1);
    p2 = bf16_rne(r2);
}

}  // namespace tik_host
