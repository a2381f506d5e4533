// stream_plan.h — the host side of an online-IK stream, with no HIP call in
// it: everything tik_stream_create decides from the model's shapes and the
// window size, before the first device call (stream.cpp executes the result).
//
//   limits    what any stream needs (window, ring, pose width); a violation is
//             TIK_E_INVALID with a message that names the value
//   coverage  what the dataflow kernel (online.hip) can run; a model outside it
//             is no error, it gets the layered step
//   plan      the dataflow step: with 3x1 temporal convs, output frame t of a
//             stride-s layer reads input frames s t - 1 .. s t + 1, so pose row 0
//             needs only the first frames of every layer. Walking that back from
//             the head gives n_out / n_in per layer; from them follow the one
//             activation buffer's layout, the task list and the counter words
//   packers   the kernel's weight layouts, as pure functions of host vectors
//   frames    what a push checks before it takes a frame (check_frame), and the
//             hold-last fill of a frame pushed with confidences (fill_frame)
//
// Stands alone in tests/test_stream_plan_host.py and tests/test_lm_robust_host.py.
#pragma once
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "fold.h"
#include "online_defs.h"

namespace tik_stream_plan {

using tik_host::fail;

constexpr int V = 17;            // COCO joints
constexpr int FRAME = V * 3;     // floats of the frame a push takes
constexpr int POSE_DIM = 66;     // floats per pose a push returns (include/tik.h, streaming.py)
constexpr int POSE_FLAG = POSE_DIM;             // the pinned pose buffer: the pose, then the dataflow kernel's
constexpr int HOST_POSE_FLOATS = POSE_DIM + 1;  // error flag (online.hip writes it at pose_dim)
constexpr int ROOT_A = 11, ROOT_B = 12;   // hips: the window is relative to their midpoint

struct LayerShape {
    int cin, cinp, cout, stride, res;   // res: ONR_*
};
struct ModelShape {
    std::vector<LayerShape> layers;
    int V = 0, C0 = 0, feat = 0, hidden = 0, pose_dim = 0;   // pose_dim 0: a backbone-only handle
};

inline int frames_out(int tin, int stride) { return stride < 1 ? 0 : (tin - 1) / stride + 1; }   // kt = 3, pad = 1
inline int steps32(int k) { return (k + 31) / 32; }
// K of a temporal conv task: the three taps, then the residual conv's input channels
inline int tconv_k(const LayerShape& l) { return 3 * l.cout + (l.res == tik::ONR_CONV ? l.cinp : 0); }

// ---------------------------------------------------------------- limits (any step)
struct Limits {
    int h = 0, W = 0;   // frames either side of the centre; ring and window size 2h + 1
    int tout = 0;       // the model's output frames for a window of W
    long long period = 0;      // 2 W: a count moved by a multiple of it keeps its ring slot and launch parity
    size_t ring_floats = 0;    // W frames: the ring, and the layered step's gathered window
    size_t poses_floats = 0;   // the layered forward's output: tout pose rows
};

inline int stream_limits(const ModelShape& m, int win_size, Limits& o) {
    if (win_size <= 0) return fail(TIK_E_INVALID, "tik_stream_create: win_size %d is not positive", win_size);
    o.h = win_size / 2;
    o.W = 2 * o.h + 1;
    o.period = 2LL * o.W;
    // stream_next_count (online.h) subtracts 2 W * (2^29 / 2 W) at the wrap: the quotient must be at least 1
    if (o.period > (1LL << 29))
        return fail(TIK_E_INVALID, "tik_stream_create: win_size %d gives a ring of %d frames, and twice that exceeds 2^29", win_size, o.W);
    o.tout = o.W;
    for (const LayerShape& l : m.layers) o.tout = frames_out(o.tout, l.stride);
    if (o.tout < 1) return fail(TIK_E_INVALID, "tik_stream_create: the model gives %d output frames for a window of %d", o.tout, o.W);
    if (m.pose_dim <= 0) return fail(TIK_E_INVALID, "tik_stream_create: backbone-only model handle");
    if (m.pose_dim != POSE_DIM)
        return fail(TIK_E_INVALID, "tik_stream_create: the model's pose width is %d (rows of pose_regressor.3); a stream returns %d floats per pose",
                    m.pose_dim, POSE_DIM);
    o.ring_floats = (size_t)o.W * FRAME;
    o.poses_floats = (size_t)o.tout * POSE_DIM;
    return TIK_OK;
}

// ---------------------------------------------------------------- the pushed frame (any step)
// Index of the first NaN or Inf among n floats, or -1. From the bits, so that no
// floating-point compile option can fold the test away.
inline int first_nonfinite(const float* f, int n) {
    for (int i = 0; i < n; ++i) {
        unsigned u;
        memcpy(&u, f + i, sizeof u);
        if ((u & 0x7f800000u) == 0x7f800000u) return i;
    }
    return -1;
}

// tik_stream_push's check, before anything is copied or enqueued: both ReLUs of the
// dataflow kernel turn a NaN into 0 (online.hip), so a non-finite frame would give a
// finite, wrong pose for every window that holds it. It is refused instead.
inline int check_frame(const float* frame) {
    const int i = first_nonfinite(frame, FRAME);
    if (i < 0) return TIK_OK;
    unsigned u;
    memcpy(&u, frame + i, sizeof u);
    return fail(TIK_E_INVALID, "tik_stream_push: frame value %d (joint %d, coordinate %d) is %s; the frame was not appended", i, i / 3, i % 3,
                (u & 0x007fffffu) ? "NaN" : "infinite");
}

// ---------------------------------------------------------------- a frame with confidences (any step)
// tik_stream_push_conf's rule, on the host before anything is copied or enqueued. Keypoint k is missing when
// conf[k] is 0 or one of its coordinates is not finite (a non-finite keypoint with positive confidence counts as
// confidence 0). The network cannot take a hole (check_frame), so a missing keypoint is filled with the last
// value this stream accepted for it, in absolute coordinates: hold-last. That is a stated rule, not a tuned
// one. A keypoint that is missing and was never seen since create or reset refuses the frame, as check_frame
// refuses a NaN; so does a confidence that is negative or not finite. A refusal changes nothing.
struct LastSeen {
    float kp[FRAME] = {};
    bool seen[V] = {};
    void clear() { *this = LastSeen{}; }
};

// frame (51) and conf (17) -> out_frame (51, finite) and out_conf (17: 0 where missing, else conf). `last` is read only.
inline int fill_frame(const float* frame, const float* conf, const LastSeen& last, float* out_frame, float* out_conf) {
    const int bad = first_nonfinite(conf, V);
    if (bad >= 0) return fail(TIK_E_INVALID, "tik_stream_push_conf: confidence %d is not finite; the frame was not appended", bad);
    for (int k = 0; k < V; ++k)
        if (!(conf[k] >= 0.f))
            return fail(TIK_E_INVALID, "tik_stream_push_conf: confidence %d is negative (%g); the frame was not appended", k, (double)conf[k]);
    for (int k = 0; k < V; ++k) {
        const bool missing = conf[k] == 0.f || first_nonfinite(frame + 3 * k, 3) >= 0;
        if (missing && !last.seen[k])
            return fail(TIK_E_INVALID, "tik_stream_push_conf: joint %d is missing and has not been seen since the stream was created or "
                        "reset; the frame was not appended", k);
        const float* src = missing ? last.kp + 3 * k : frame + 3 * k;
        for (int c = 0; c < 3; ++c) out_frame[3 * k + c] = src[c];
        out_conf[k] = missing ? 0.f : conf[k];
    }
    return TIK_OK;
}

// the frame the stream accepted (finite: check_frame or fill_frame passed) becomes the last value of every keypoint
// (a filled one repeats what was held, so after any accepted frame every keypoint has been seen)
inline void accept_frame(LastSeen& last, const float* frame) {
    for (int k = 0; k < V; ++k) last.seen[k] = true;
    memcpy(last.kp, frame, sizeof last.kp);
}

// ---------------------------------------------------------------- the dataflow step
struct LayerPlan {
    int tin = 0;                // the layer's real input frame count (zero padding past it)
    int n_in = 0, n_out = 0;    // frames computed: z (gcn) / out (temporal conv)
    int k32 = 0, gk32 = 0;      // temporal conv K / gcn K in steps of 32
    long long x = -1;           // float offsets in the activation buffer: the input rows (the layer
    long long z = 0, out = 0;   // before's out; -1: layer 0 builds them from the ring), z and out
};

struct Counters {   // the scheduling words, as offsets into one int buffer
    int cnt = 0, ncnt = 0;   // one completion counter per head phase (G / T hand over tagged data)
    int ticket = 0, done = 0, err = 0;
    int words = 0;
};

struct Plan {
    std::vector<LayerPlan> L;
    long long hpart = 0, pose = 0;   // [hidden / 16][pose_dim] shares of pose_regressor.3; the pose row
    long long act_floats = 0;
    unsigned act_bytes = 0;          // below 2^31: the kernel's buffer resource takes it as an int
    int trace_words = 0;             // TIK_ONLINE_TRACE: 8 words per task
    std::vector<tik::OnlinePhase> ph;
    int ntasks = 0;
    Counters c;
};

// "" when online.hip covers the model, else the reason it does not
inline std::string coverage(const ModelShape& m) {
    char b[160] = "";
    const int nl = (int)m.layers.size();
    if (m.V != V || m.C0 != 3 || nl < 1 || nl > tik::ONL_MAXL) {
        snprintf(b, sizeof b, "V=17, 3 input channels, 1..%d layers", tik::ONL_MAXL);
        return b;
    }
    for (int l = 0; l < nl; ++l) {
        const LayerShape& L = m.layers[l];
        if (L.cout <= 0 || L.cout % 16 || L.cout > tik::ONL_MAXC || L.cinp > tik::ONL_MAXC || (l > 0 && L.cinp != L.cin) || L.stride < 1) {
            snprintf(b, sizeof b, "layer %d channels %d -> %d, stride %d", l, L.cin, L.cout, L.stride);
            return b;
        }
    }
    // head tasks: one thread per pose value, W3 columns in LDS
    if (m.feat % 4 || m.feat > tik::ONL_MAXHC * 256 || m.hidden % 16 || m.hidden > tik::ONL_MAXHC * 256 || m.pose_dim > 256) {
        snprintf(b, sizeof b, "head %d -> %d -> %d", m.feat, m.hidden, m.pose_dim);
        return b;
    }
    if (2 * nl + 1 > tik::ONL_MAXPH) return "too many phases";
    return "";
}

// The plan of a covered model (coverage(m) is empty). false: the activation buffer
// would pass the 2^31 bytes of the kernel's buffer resource (p is then unspecified).
inline bool plan_dataflow(const ModelShape& m, const Limits& lim, Plan& p) {
    const int nl = (int)m.layers.size();
    p = Plan{};
    p.L.resize(nl);
    int t = lim.W;
    for (int l = 0; l < nl; ++l) {
        p.L[l].tin = t;
        t = frames_out(t, m.layers[l].stride);
        p.L[l].k32 = steps32(tconv_k(m.layers[l]));
        p.L[l].gk32 = steps32(m.layers[l].cinp);
    }
    long long need = 1;   // the last layer's output frames: row 0
    for (int l = nl - 1; l >= 0; --l) {
        p.L[l].n_out = (int)need;
        need = std::min<long long>(p.L[l].tin, m.layers[l].stride * (need - 1) + 2);
        p.L[l].n_in = (int)need;
    }
    long long q = 0;
    for (int l = 0; l < nl; ++l) {
        LayerPlan& L = p.L[l];
        L.x = l == 0 ? -1 : p.L[l - 1].out;
        L.z = q; q += (long long)L.n_in * V * m.layers[l].cout;
        L.out = q; q += (long long)L.n_out * V * m.layers[l].cout;
    }
    p.hpart = q; q += (long long)(m.hidden / 16) * m.pose_dim;
    p.pose = q; q += (m.pose_dim + 3) & ~3;
    p.act_floats = q;
    if (q * (long long)sizeof(float) >= (1LL << 31)) return false;
    p.act_bytes = (unsigned)(q * sizeof(float));
    // tasks in topological order; their number is below act_floats
    auto add = [&p](int kind, int layer, int nf, int ng) {
        p.ph.push_back(tik::OnlinePhase{kind, layer, nf, ng, p.ntasks, p.c.ncnt});
        p.ntasks += nf * ng;
        if (kind == tik::ONP_H) ++p.c.ncnt;
    };
    for (int l = 0; l < nl; ++l) {
        add(tik::ONP_G, l, p.L[l].n_in, m.layers[l].cout / 16);
        add(tik::ONP_T, l, p.L[l].n_out, m.layers[l].cout / 16);
    }
    add(tik::ONP_H, nl - 1, 1, m.hidden / 16);
    p.trace_words = 8 * p.ntasks;
    p.c.cnt = 0;
    p.c.ticket = p.c.ncnt;
    p.c.done = p.c.ncnt + 1;
    p.c.err = p.c.ncnt + 2;
    p.c.words = p.c.ncnt + 3;
    return true;
}

// ---------------------------------------------------------------- weight packers
// The temporal conv task's rows: K = [tap 0 | tap 1 | tap 2 | residual conv] per output
// channel. wt [cout][3 cout]; wr [cout][cinp], read only when the layer has a residual conv.
inline std::vector<float> concat_k(const LayerShape& l, const std::vector<float>& wt, const std::vector<float>& wr) {
    const int C = l.cout, Kt = tconv_k(l);
    std::vector<float> w((size_t)C * Kt);
    for (int co = 0; co < C; ++co)
        for (int k = 0; k < Kt; ++k)
            w[(size_t)co * Kt + k] = k < 3 * C ? wt[(size_t)co * 3 * C + k] : wr[(size_t)co * l.cinp + (k - 3 * C)];
    return w;
}

// rows [cout][Kt] -> wf: fp32 rows zero-padded to steps32(Kt) steps of 32; wp: their bf16x3
// planes [cout/16][K32][3][64][8] in the MFMA B-operand lane layout (lane ln holds row
// 16 cg + ln % 16, K 32 sk + 8 (ln / 16) .. + 7)
inline void pack_rows(const std::vector<float>& w, int cout, int Kt, std::vector<float>& wf, std::vector<unsigned short>& wp) {
    const int K32 = steps32(Kt);
    wf.assign((size_t)cout * 32 * K32, 0.f);
    for (int co = 0; co < cout; ++co)
        for (int k = 0; k < Kt; ++k) wf[(size_t)co * 32 * K32 + k] = w[(size_t)co * Kt + k];
    wp.assign((size_t)(cout / 16) * K32 * 3 * 64 * 8, 0);
    for (int cg = 0; cg < cout / 16; ++cg)
        for (int sk = 0; sk < K32; ++sk)
            for (int ln = 0; ln < 64; ++ln)
                for (int e = 0; e < 8; ++e) {
                    unsigned short h[3];
                    tik_host::split_bf16x3(wf[(size_t)(16 * cg + (ln & 15)) * 32 * K32 + 32 * sk + 8 * (ln >> 4) + e], h[0], h[1], h[2]);
                    for (int pl = 0; pl < 3; ++pl) wp[((((size_t)cg * K32 + sk) * 3 + pl) * 64 + ln) * 8 + e] = h[pl];
                }
}

}  // namespace tik_stream_plan
