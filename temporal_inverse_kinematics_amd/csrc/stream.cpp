// stream.cpp — the online (stride-1 sliding-window) IK handle (BASELINE.json
// config #5). The reference solves a recorded sequence offline, one window per
// frame (inference.run_inference, inference.py:37-67; windows from
// data_amass.py:18-42, 221-236). Online, frame c can be solved once frame c+h
// has arrived: each push of frame k runs the window centred at c = k-h (frames
// k-2h..k, left edge clamped like sample_window's edge padding) and returns
// pose row 0 of the model output, i.e. exactly run_inference's frame c.
// Flushing the last h frames = pushing the last frame h more times (right edge
// padding).
//
// tik_stream_create plans on the host first (stream_plan.h: the stream's
// limits, whether the dataflow kernel covers the model, that step's layout), so
// a refused model or window allocates nothing and never touches the GPU; then
// it allocates what the one recorded step needs (stream_step.cpp) and captures
// it into a hipGraph on a private stream when use_graph. Also here: reset,
// destroy and the debug hooks.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <memory>
#include <new>
#include <type_traits>

#include "stream.h"

using namespace tik_host;
namespace sp = tik_stream_plan;

namespace {

struct StreamEnv {   // read once, at create
    bool online;     // TIK_ONLINE=0: the layered step whatever the model
    bool trace;      // TIK_ONLINE_TRACE=1: per-task time stamps (tik_debug_stream_trace)
    int grid_cap;    // TIK_ONLINE_GRID: at most this many workgroups (test hook)
};
StreamEnv read_env() {
    const char *o = getenv("TIK_ONLINE"), *t = getenv("TIK_ONLINE_TRACE"), *g = getenv("TIK_ONLINE_GRID");
    return StreamEnv{!(o && o[0] == '0'), t && t[0] == '1', g ? atoi(g) : INT_MAX};
}

// every G / T output carries its launch's tag in its sign bit (online.hip): tag 1 before launch 0
constexpr int ACT_TAG1 = (int)0x80000000u;
constexpr int CONF_ONE = 0x3f800000;   // 1.0f: the confidence of a frame pushed without one

template <class T>
int host_alloc(T** p, size_t n, unsigned flags) {
    void* q = nullptr;
    HIP_TRY(hipHostMalloc(&q, n * sizeof(T), flags));
    *p = static_cast<T*>(q);
    return TIK_OK;
}

// the device's address of a pinned host word
template <class T, class U>
int device_view(T** dev, U* pinned) {
    void* q = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&q, const_cast<std::remove_cv_t<U>*>(pinned), 0));
    *dev = static_cast<T*>(q);
    return TIK_OK;
}

// what either step needs: the private stream, the ring and its count (zero), the pinned words
int alloc_common(tik_stream* s) {
    int rc;
    if ((rc = s->ring.reserve(s->lim.ring_floats)) || (rc = s->count.reserve(1))) return rc;
    HIP_TRY(hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking));
    int* done = nullptr;
    if ((rc = host_alloc(&s->host_frame, sp::FRAME, hipHostMallocDefault)) ||
        (rc = host_alloc(&s->host_pose, sp::HOST_POSE_FLOATS, hipHostMallocCoherent)) || (rc = host_alloc(&done, 1, hipHostMallocCoherent)))
        return rc;
    s->host_done = done;
    s->host_pose[sp::POSE_FLAG] = 0.f;
    *s->host_done = 0;
    HIP_TRY(hipMemsetAsync(s->count.p, 0, sizeof(int), s->st));
    HIP_TRY(hipMemsetAsync(s->ring.p, 0, sizeof(float) * s->ring.n, s->st));
    return TIK_OK;
}

int alloc_layered(tik_stream* s) {
    int rc;
    if ((rc = model_reserve_ws(s->model, s->ws, 1, s->lim.W)) || (rc = s->window.reserve(s->lim.ring_floats)) ||
        (rc = s->poses.reserve(s->lim.poses_floats)) || (rc = s->frame_in.reserve(sp::FRAME)))
        return rc;
    return TIK_OK;
}

int download(std::vector<float>& h, const float* dev) {
    if (!h.empty()) HIP_TRY(hipMemcpy(h.data(), dev, h.size() * sizeof(float), hipMemcpyDeviceToHost));
    return TIK_OK;
}

// the dataflow step's buffers, its repacked weights and the kernel's argument block: the plan, copied
int alloc_dataflow(tik_stream* s, const OnlineModelView& v, const sp::Plan& p, const StreamEnv& env) {
    const int nl = (int)p.L.size();
    int rc;
    if ((rc = s->onl_act.reserve((size_t)p.act_floats)) || (rc = s->onl_cnt.reserve(p.c.words)) ||
        (env.trace && (rc = s->onl_trace.reserve(p.trace_words))))
        return rc;
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(s->onl_act.p), ACT_TAG1, s->onl_act.n, s->st));
    HIP_TRY(hipMemsetAsync(s->onl_cnt.p, 0, sizeof(int) * s->onl_cnt.n, s->st));
    auto act = [s](long long off) { return off < 0 ? nullptr : s->onl_act.p + off; };
    tik::OnlineArgs a{};
    a.nl = nl; a.nph = (int)p.ph.size(); a.ntasks = p.ntasks;
    std::copy(p.ph.begin(), p.ph.end(), a.ph);
    s->onl_wtp.resize(nl); s->onl_wtf.resize(nl); s->onl_wgp.resize(nl); s->onl_wgf.resize(nl);
    for (int l = 0; l < nl; ++l) {
        // the weights start from the model's folded fp32 rows, copied back from the device
        const sp::LayerShape& sh = v.shape.layers[l];
        const bool rconv = sh.res == tik::ONR_CONV;
        std::vector<float> wt((size_t)sh.cout * 3 * sh.cout), wr(rconv ? (size_t)sh.cout * sh.cinp : 0), wg((size_t)sh.cout * sh.cinp), wf;
        std::vector<unsigned short> wp;
        if ((rc = download(wt, v.L[l].wt)) || (rc = download(wr, v.L[l].wr)) || (rc = download(wg, v.L[l].wg))) return rc;
        sp::pack_rows(sp::concat_k(sh, wt, wr), sh.cout, sp::tconv_k(sh), wf, wp);
        if ((rc = s->onl_wtp[l].upload(wp)) || (rc = s->onl_wtf[l].upload(wf))) return rc;
        sp::pack_rows(wg, sh.cout, sh.cinp, wf, wp);
        if ((rc = s->onl_wgp[l].upload(wp)) || (rc = s->onl_wgf[l].upload(wf))) return rc;
        tik::OnlineLayer& L = a.L[l];
        L.cinp = sh.cinp; L.cout = sh.cout; L.stride = sh.stride; L.res = sh.res;
        L.tin = p.L[l].tin;
        L.bias2 = v.L[l].bias2; L.amix = v.L[l].amix; L.biasT = v.L[l].biasT;
        L.gk32 = p.L[l].gk32; L.wgp = s->onl_wgp[l].p; L.wgf = s->onl_wgf[l].p;
        L.k32 = p.L[l].k32; L.wtp = s->onl_wtp[l].p; L.wtf = s->onl_wtf[l].p;
        L.x = act(p.L[l].x); L.z = act(p.L[l].z); L.out = act(p.L[l].out);
    }
    a.ring = s->ring.p; a.W = s->lim.W; a.h = s->lim.h; a.ra = sp::ROOT_A; a.rb = sp::ROOT_B; a.relative = 1;
    a.count = s->count.p;
    a.bn_sc = v.bn_sc; a.bn_sh = v.bn_sh;
    a.w0 = v.w0; a.b0 = v.b0; a.w3 = v.w3; a.b3 = v.b3;
    a.feat = v.shape.feat; a.hidden = v.shape.hidden; a.pose_dim = v.shape.pose_dim;
    a.hpart = act(p.hpart); a.pose = act(p.pose);
    s->onl_pose = a.pose;
    if ((rc = device_view(&a.frame, s->host_frame)) || (rc = device_view(&a.pose_host, s->host_pose)) ||
        (rc = device_view(&a.done_host, s->host_done)))
        return rc;
    a.cnt = s->onl_cnt.p + p.c.cnt; a.ncnt = p.c.ncnt;
    a.ticket = s->onl_cnt.p + p.c.ticket; a.done = s->onl_cnt.p + p.c.done; a.err = s->onl_cnt.p + p.c.err;
    a.trace = s->onl_trace.p;
    a.act = s->onl_act.p; a.act_bytes = p.act_bytes;
    if ((rc = s->onl_args.upload(std::vector<tik::OnlineArgs>{a}))) return rc;
    s->onl_c = p.c;
    s->onl_ntasks = p.ntasks;
    // one workgroup per CU (89 KB of LDS each). With per-frame counters half the CUs was best
    // (143 us at 128 vs 151 us at 256); with tagged data the wider grid wins: p50 81 us at 128,
    // 74 at 160, 70 at 192, 67 at 256 (profiles/r05_og_ab_online_grid.txt)
    s->onl_grid = std::max(1, std::min(v.ncu, env.grid_cap));
    return TIK_OK;
}

int capture_step(tik_stream* s) {
    // a step recorded before (tik_stream_set_refine records again): idle by now, its graph goes
    if (s->exec) HIP_TRY(hipGraphExecDestroy(s->exec));
    if (s->graph) HIP_TRY(hipGraphDestroy(s->graph));
    s->exec = nullptr;
    s->graph = nullptr;
    HIP_TRY(hipStreamBeginCapture(s->st, hipStreamCaptureModeThreadLocal));
    const int rc = stream_record_step(s);
    const hipError_t e = hipStreamEndCapture(s->st, &s->graph);   // the handle owns the graph from here
    if (rc) return rc;
    if (e != hipSuccess) return fail(TIK_E_HIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
    HIP_TRY(hipGraphInstantiate(&s->exec, s->graph, nullptr, nullptr, 0));
    return TIK_OK;
}

}  // namespace

extern "C" {

int tik_stream_create(tik_model_t model, int win_size, int use_graph, tik_stream_t* out) try {
    if (!model || !out) return fail(TIK_E_INVALID, "tik_stream_create: null argument");
    *out = nullptr;
    // host: a refused model or window allocates nothing and never touches the GPU
    const StreamEnv env = read_env();
    const OnlineModelView v = model_online_view(model);
    sp::Limits lim;
    sp::Plan plan;
    int rc;
    if ((rc = sp::stream_limits(v.shape, win_size, lim))) return rc;
    // a model the dataflow kernel does not cover is no error: it runs the layered step
    const bool online = env.online && sp::coverage(v.shape).empty() && sp::plan_dataflow(v.shape, lim, plan);
    // device
    auto s = std::make_unique<tik_stream>();
    model_retain(model);
    s->model = model;
    s->lim = lim;
    s->online = online;
    if ((rc = alloc_common(s.get())) || (rc = online ? alloc_dataflow(s.get(), v, plan, env) : alloc_layered(s.get()))) return rc;
    // ring, count, the initial tags and the scheduling words are in place before the first step
    // on this (non-blocking) stream: the memsets ran on it, and the host waits here
    HIP_TRY(hipStreamSynchronize(s->st));
    if (use_graph && (rc = capture_step(s.get()))) return rc;
    *out = s.release();
    return TIK_OK;
} catch (const std::bad_alloc&) {   // the plan and the repack live in host vectors; no exception crosses the C ABI
    return fail(TIK_E_NOMEM, "tik_stream_create: out of host memory");
}

int tik_stream_destroy(tik_stream_t s) {
    const std::unique_ptr<tik_stream> owned(s);   // what create released; null is fine
    return TIK_OK;
}

int tik_stream_path(tik_stream_t s) {
    if (!s) return fail(TIK_E_INVALID, "null stream");
    return s->online ? 1 : 0;
}

int tik_debug_stream_trace(tik_stream_t s, long long* out, int cap) {
    if (!s || !s->online || !s->onl_trace.p) return fail(TIK_E_INVALID, "no online trace (TIK_ONLINE_TRACE=1 at tik_stream_create)");
    const int n = std::min(cap / 8, s->onl_ntasks);
    // a push returns once the pose is in host memory, while the launch's tail (the last
    // tasks' end marks, the scheduling bookkeeping) may still run on the non-blocking
    // stream, which a null-stream copy does not wait for
    HIP_TRY(hipStreamSynchronize(s->st));
    if (out && n > 0) HIP_TRY(hipMemcpy(out, s->onl_trace.p, sizeof(long long) * 8 * n, hipMemcpyDeviceToHost));
    return s->onl_ntasks;
}

int tik_stream_reset(tik_stream_t s) {
    if (!s) return fail(TIK_E_INVALID, "null stream");
    HIP_TRY(hipMemsetAsync(s->count.p, 0, sizeof(int), s->st));
    if (s->online) {
        // the dataflow kernel's scheduling state: completion counters, ticket, done, err
        HIP_TRY(hipMemsetAsync(s->onl_cnt.p, 0, sizeof(int) * s->onl_c.words, s->st));
        // count restarts at 0: the activations go back to tag 1 (online.hip)
        HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(s->onl_act.p), ACT_TAG1, s->onl_act.n, s->st));
    }
    if (s->rhave.p) HIP_TRY(hipMemsetAsync(s->rhave.p, 0, sizeof(int), s->st));   // no previous refined pose
    HIP_TRY(hipStreamSynchronize(s->st));
    s->host_pose[sp::POSE_FLAG] = 0.f;
    *s->host_done = 0;
    if (s->host_rdone) *s->host_rdone = 0;
    s->pushed = 0;
    s->dcount = 0;
    s->last.clear();   // no keypoint has been seen; the confidence ring's slots are written before they are read
    return TIK_OK;
}

int tik_stream_set_robust(tik_stream_t s, float sigma) {
    if (!s) return fail(TIK_E_INVALID, "tik_stream_set_robust: null stream");
    if (int rc = tik::lm_refine_check_sigma("tik_stream_set_robust", sigma)) return rc;
    HIP_TRY(hipStreamSynchronize(s->st));   // idle between pushes
    s->rsigma = sigma;
    if (!s->refining()) return TIK_OK;      // kept for a later tik_stream_set_refine
    s->rargs.sigma = sigma;
    return s->exec ? capture_step(s) : TIK_OK;
}

int tik_stream_set_refine(tik_stream_t s, tik_fk_t fk, const float* betas_host, const float* joint_w_host, int iters, float mu,
                          float smooth, float lam0) try {
    if (!s) return fail(TIK_E_INVALID, "tik_stream_set_refine: null stream");
    // host: a refused setting leaves the stream as it was
    tik::LmRefineArgs a{};
    if (iters != 0) {
        if (int rc = tik::lm_refine_model_args(fk, "tik_stream_set_refine", nullptr, iters, mu, smooth, lam0, a)) return rc;
        if (joint_w_host)
            for (int k = 0; k < tik::LMR_COLS; ++k)
                if (!(joint_w_host[k] >= 0.f))
                    return fail(TIK_E_INVALID, "tik_stream_set_refine: joint weight %d must be >= 0, got %g", k, (double)joint_w_host[k]);
    }
    // device: the stream is idle between pushes; the step is recorded again with or without the extra launch
    HIP_TRY(hipStreamSynchronize(s->st));
    const bool graph = s->exec != nullptr;
    int rc;
    if (iters != 0) {
        int* done = nullptr;
        if ((betas_host && a.nb > 0 && (rc = s->rbetas.upload(std::vector<float>(betas_host, betas_host + a.nb)))) ||
            (joint_w_host && (rc = s->rjw.upload(std::vector<float>(joint_w_host, joint_w_host + tik::LMR_COLS)))) ||
            (rc = s->rprev.reserve(tik::LMR_N)) || (rc = s->rhave.reserve(1)) ||
            (rc = s->cring.reserve((size_t)s->lim.W * tik::LMR_COLS)) ||
            (!s->host_conf && (rc = host_alloc(&s->host_conf, tik::LMR_COLS, hipHostMallocDefault))) ||
            (!s->host_refined && (rc = host_alloc(&s->host_refined, tik::LMR_N, hipHostMallocCoherent))) ||
            (!s->host_rdone && ((rc = host_alloc(&done, 1, hipHostMallocCoherent)) || (s->host_rdone = done, 0))))
            return rc;
        HIP_TRY(hipMemsetAsync(s->rhave.p, 0, sizeof(int), s->st));
        HIP_TRY(hipMemsetAsync(s->rprev.p, 0, sizeof(float) * tik::LMR_N, s->st));
        // the frames already in the ring were pushed without the refine launch: confidence one
        HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(s->cring.p), CONF_ONE, s->cring.n, s->st));
        HIP_TRY(hipStreamSynchronize(s->st));
        for (int k = 0; k < tik::LMR_COLS; ++k) s->host_conf[k] = 1.f;
        *s->host_rdone = s->dcount;
        a.B = 1;
        a.poses = s->online ? s->onl_pose : s->poses.p;   // the step's device copy of pose row 0 (the dataflow kernel's carries no tag)
        a.betas = betas_host && a.nb > 0 ? s->rbetas.p : nullptr;
        a.joint_w = joint_w_host ? s->rjw.p : nullptr;
        a.st.count = s->count.p; a.st.ring = s->ring.p; a.st.W = s->lim.W; a.st.h = s->lim.h;
        a.st.prev = s->rprev.p; a.st.have = s->rhave.p;
        a.st.cring = s->cring.p;
        a.sigma = s->rsigma;
        if ((rc = device_view(&a.st.pose_host, s->host_refined)) || (rc = device_view(&a.st.done_host, s->host_rdone)) ||
            (rc = device_view(&a.st.conf_host, s->host_conf)))
            return rc;
        fk_retain(fk);
    }
    if (s->rfk) fk_release(s->rfk);
    s->rfk = iters != 0 ? fk : nullptr;
    s->rargs = a;
    return graph ? capture_step(s) : TIK_OK;
} catch (const std::bad_alloc&) {
    return fail(TIK_E_NOMEM, "tik_stream_set_refine: out of host memory");
}

int tik_debug_stream_inject_error(tik_stream_t s) {
    if (!s || !s->online) return fail(TIK_E_INVALID, "tik_debug_stream_inject_error: not a dataflow-kernel stream");
    const int one = 1;
    HIP_TRY(hipMemcpyAsync(s->onl_cnt.p + s->onl_c.err, &one, sizeof(int), hipMemcpyHostToDevice, s->st));
    HIP_TRY(hipStreamSynchronize(s->st));
    return TIK_OK;
}

int tik_debug_stream_set_count(tik_stream_t s, int count) {
    if (!s) return fail(TIK_E_INVALID, "null stream");
    const long long period = s->lim.period;
    if (count < 0 || count >= (1 << 30) || ((long long)count - s->dcount) % period != 0)
        return fail(TIK_E_INVALID, "tik_debug_stream_set_count: %d is not the current count %d modulo %lld (or out of range)",
                    count, s->dcount, period);
    HIP_TRY(hipStreamSynchronize(s->st));
    HIP_TRY(hipMemcpy(s->count.p, &count, sizeof(int), hipMemcpyHostToDevice));
    s->dcount = count;
    return TIK_OK;
}

}  // extern "C"
