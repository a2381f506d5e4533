// stream.h — the online-IK stream handle, shared by stream.cpp (create: plan
// on the host with stream_plan.h, then allocate; reset, destroy, debug hooks)
// and stream_step.cpp (the recorded step and tik_stream_push), and what
// model.cpp hands a stream: shapes and device pointers, nothing else.
#pragma once
#include "common.h"
#include "fk_model.h"
#include "lm_refine.h"
#include "online.h"
#include "stream_plan.h"

namespace tik_host {

struct OnlineModelView {
    tik_stream_plan::ModelShape shape;
    struct LayerPtrs {
        const float *wg, *bias2, *amix, *wt, *wr, *biasT;   // the folded fp32 weights of model.h's Layer
    };
    std::vector<LayerPtrs> L;
    const float *bn_sc = nullptr, *bn_sh = nullptr, *w0 = nullptr, *b0 = nullptr, *w3 = nullptr, *b3 = nullptr;
    int ncu = 0;   // compute units
};
OnlineModelView model_online_view(const tik_model* m);   // model.cpp

// the step a stream records (stream_step.cpp)
int stream_record_step(tik_stream* s);

}  // namespace tik_host

struct tik_stream {
    tik_model_t model = nullptr;   // retained: the handle may be destroyed first
    tik_stream_plan::Limits lim;   // h, W, tout
    hipStream_t st = nullptr;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    tik_host::DevBuf ring;         // W frames
    tik_host::DevIBuf count;       // frames pushed so far (stream_next_count)
    float* host_frame = nullptr;   // pinned
    float* host_pose = nullptr;    // pinned; [POSE_FLAG] = the online kernel's error flag
    volatile int* host_done = nullptr;   // pinned, coherent: the dataflow kernel's frame count after each step
    long long pushed = 0;
    int dcount = 0;                // mirror of the device frame count
    bool online = false;           // which of the two steps below is the one recorded
    // the layered step: ring append, window gather, the IK forward on (1, W), the pose copy
    tik_host::Workspace ws;        // private: batch calls on the handle never touch it
    tik_host::DevBuf window, poses, frame_in;
    // the dataflow step (online.hip)
    int onl_grid = 0;
    tik_stream_plan::Counters onl_c;               // where onl_cnt's words are
    int onl_ntasks = 0;
    tik_host::DevBuf onl_act;                      // every activation of the step
    tik_host::DevIBuf onl_cnt;                     // completion counters, ticket, done, err
    tik_host::DevArray<tik::OnlineArgs> onl_args;  // the kernel's argument block
    tik_host::DevArray<unsigned long long> onl_trace;   // TIK_ONLINE_TRACE=1
    std::vector<tik_host::DevHBuf> onl_wtp, onl_wgp;    // per layer: temporal conv / gcn weights as bf16x3 MFMA planes
    std::vector<tik_host::DevBuf> onl_wtf, onl_wgf;     // per layer: the same, fp32, K zero-padded to 32
    float* onl_pose = nullptr;                     // the dataflow step's device copy of the pose row (inside onl_act; no tag)
    // the refinement launch that follows either step (tik_stream_set_refine; lm_refine.hip, B = 1)
    tik_fk_t rfk = nullptr;        // retained while the stream refines with it
    tik::LmRefineArgs rargs{};     // the launch's arguments; rargs.iters == 0: no refinement
    tik_host::DevBuf rbetas, rjw, rprev;   // betas (nb), keypoint weights (17), the previous refined pose (66)
    tik_host::DevIBuf rhave;       // non-zero once rprev holds a pose
    float rsigma = 0.f;            // tik_stream_set_robust's scale; copied into rargs whenever the step is recorded
    tik_host::DevBuf cring;        // W rows of 17 confidences beside the ring (a refining stream's)
    float* host_conf = nullptr;    // pinned: this push's confidences, read by the refine launch (ones for a plain push)
    tik_stream_plan::LastSeen last;   // per keypoint, the last value the stream accepted (tik_stream_push_conf's fill)
    float* host_refined = nullptr;         // pinned, coherent: the refined pose
    volatile int* host_rdone = nullptr;    // pinned, coherent: the frame count after each refined step
    bool refining() const { return rargs.iters > 0; }
    ~tik_stream() {
        if (st) (void)hipStreamSynchronize(st);
        if (exec) (void)hipGraphExecDestroy(exec);
        if (graph) (void)hipGraphDestroy(graph);
        if (host_frame) (void)hipHostFree(host_frame);
        if (host_pose) (void)hipHostFree(host_pose);
        if (host_done) (void)hipHostFree(const_cast<int*>(host_done));
        if (host_refined) (void)hipHostFree(host_refined);
        if (host_conf) (void)hipHostFree(host_conf);
        if (host_rdone) (void)hipHostFree(const_cast<int*>(host_rdone));
        if (st) (void)hipStreamDestroy(st);
        if (model) tik_host::model_release(model);
        if (rfk) tik_host::fk_release(rfk);
    }
};
