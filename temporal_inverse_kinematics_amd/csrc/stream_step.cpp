// stream_step.cpp — the step an online-IK stream records and tik_stream_push.
// Default step: ONE dataflow kernel (online.hip) that reads the frame from
// pinned host memory, appends it to the ring, computes only the frames pose
// row 0 depends on, and writes the pose to pinned host memory. Layered step
// (TIK_ONLINE=0, or a model that kernel does not cover, stream_plan.h): ring
// append, window gather, the layered IK forward on the whole window, the pose
// copy. Either is one hipGraph replay on the private stream when the stream
// was created with use_graph (stream.cpp). tik_stream_push_conf is the same push
// behind the host fill of stream_plan.h (fill_frame): the frame it hands on is
// finite, and its 17 confidences go to pinned memory for the refine launch.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>

#include "misc.h"
#include "stream.h"

using namespace tik_host;
namespace sp = tik_stream_plan;

namespace tik_host {

// the refinement of the frame the step just solved: one more launch in stream order, the same kernel as tik_fk_refine
static int record_refine(tik_stream* s) {
    return s->refining() ? tik::lm_refine_launch(s->rargs, s->st) : TIK_OK;
}

int stream_record_step(tik_stream* s) {
    if (s->online) {
        HIP_TRY(tik::launch_online(s->onl_args.p, s->onl_grid, s->st));
        return record_refine(s);
    }
    HIP_TRY(hipMemcpyAsync(s->frame_in.p, s->host_frame, sizeof(float) * sp::FRAME, hipMemcpyHostToDevice, s->st));
    HIP_TRY(tik::launch_stream_push(s->ring.p, s->lim.W, sp::FRAME, s->count.p, s->frame_in.p, s->st));
    HIP_TRY(tik::launch_stream_window(s->ring.p, s->lim.W, sp::V, s->count.p, s->lim.h, sp::ROOT_A, sp::ROOT_B, 1, s->window.p, s->st));
    int rc = model_forward_ws(s->model, s->window.p, 1, s->lim.W, s->poses.p, s->st, s->ws, false);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(s->host_pose, s->poses.p, sizeof(float) * sp::POSE_DIM, hipMemcpyDeviceToHost, s->st));
    return record_refine(s);
}

}  // namespace tik_host

// one step on a frame that passed its check: frame (51, finite) and, for a refining stream, conf (17) or null = ones
static int push_frame(tik_stream_t s, const float* frame, const float* conf, float* pose_host) {
    sp::accept_frame(s->last, frame);
    memcpy(s->host_frame, frame, sizeof(float) * sp::FRAME);
    if (s->host_conf)
        for (int k = 0; k < sp::V; ++k) s->host_conf[k] = conf ? conf[k] : 1.f;
    if (s->exec) {
        HIP_TRY(hipGraphLaunch(s->exec, s->st));
    } else {
        int rc = stream_record_step(s);
        if (rc) return rc;
    }
    const int next = tik::stream_next_count(s->dcount, s->lim.W);
    bool seen = false;
    if (s->online || s->refining()) {
        // the dataflow kernel's last head task writes the new frame count to pinned
        // host memory after the pose: spin on it (sooner than the completion signal
        // hipStreamSynchronize waits for); the stream stays ordered for the next step.
        // A refining stream's last launch does the same with its own word, on either path.
        volatile int* done = s->refining() ? s->host_rdone : s->host_done;
        const auto t0 = std::chrono::steady_clock::now();
        for (long it = 0;; ++it) {
            if (*done == next) { seen = true; break; }
            if ((it & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) break;
        }
    }
    if (!seen) HIP_TRY(hipStreamSynchronize(s->st));
    ++s->pushed;   // the step appended the frame to the device ring either way
    s->dcount = next;
    if (s->online && s->host_pose[sp::POSE_FLAG] != 0.f) {
        s->host_pose[sp::POSE_FLAG] = 0.f;
        return fail(TIK_E_HIP, "tik_stream_push: the online kernel timed out waiting on a dependency "
                               "(this frame's pose is invalid; the stream stays usable)");
    }
    const int valid = s->pushed > s->lim.h;   // frame pushed-1-h >= 0 solved
    if (valid && pose_host) memcpy(pose_host, s->refining() ? s->host_refined : s->host_pose, sizeof(float) * sp::POSE_DIM);
    return valid;
}

extern "C" int tik_stream_push(tik_stream_t s, const float* frame_host, float* pose_host) {
    if (!s || !frame_host) return fail(TIK_E_INVALID, "tik_stream_push: bad arguments");
    // a NaN or Inf is refused here: nothing is copied or enqueued, ring, count and tags stay as they were
    if (const int rc = sp::check_frame(frame_host)) return rc;
    return push_frame(s, frame_host, nullptr, pose_host);
}

extern "C" int tik_stream_push_conf(tik_stream_t s, const float* frame_host, const float* conf_host, float* pose_host) {
    if (!s || !frame_host || !conf_host) return fail(TIK_E_INVALID, "tik_stream_push_conf: bad arguments");
    // the fill on the host (stream_plan.h): the ring never holds a non-finite value; a refusal changes nothing
    float frame[sp::FRAME], conf[sp::V];
    if (const int rc = sp::fill_frame(frame_host, conf_host, s->last, frame, conf)) return rc;
    return push_frame(s, frame, conf, pose_host);
}

extern "C" int tik_stream_raw_pose(tik_stream_t s, float* pose_host) {
    if (!s || !pose_host) return fail(TIK_E_INVALID, "tik_stream_raw_pose: bad arguments");
    if (s->pushed <= s->lim.h) return fail(TIK_E_INVALID, "tik_stream_raw_pose: no push has returned a pose yet");
    // either step's pose is in pinned host memory before the push that produced it returns
    memcpy(pose_host, s->host_pose, sizeof(float) * sp::POSE_DIM);
    return TIK_OK;
}
