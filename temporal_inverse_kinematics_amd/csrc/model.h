// model.h — the IK forward's handles, shared by model.cpp (fold, pack,
// reserve), forward.cpp (the launch sequence), debug.cpp (guards, checksums,
// profiler scope, traces) and api.cpp (the thin C ABI).
#pragma once
#include <atomic>
#include <string>
#include <vector>

#include "cgemm.h"
#include "common.h"
#include "xblock.h"
#include "xgemm.h"
#include "xgraph.h"

namespace tik_host {

// ---------------------------------------------------------------- algorithmic work
// FLOPs and bytes of a launch, from its shapes: what
// bench.py's roofline divides by. px = frames x joints.
struct Work {
    double flops = 0, bytes = 0;
    Work operator+(const Work& o) const { return Work{flops + o.flops, bytes + o.bytes}; }
};
enum GcnIo {
    GCN_LAYER = 0,   // reads x, weights and graph, writes z
    GCN_RAW0 = 1,    // layer 0 from the raw keypoints: the weights are not counted
    GCN_FUSED = 2,   // inside the previous block's temporal conv: x is not re-read
};
inline Work gcn_work(double px, int cin, int cout, int V, GcnIo io = GCN_LAYER) {
    const double x = io == GCN_FUSED ? 0.0 : px * cin;
    const double w = io == GCN_RAW0 ? 0.0 : (double)cout * cin + (double)V * (V + cout);
    return Work{2.0 * px * cin * cout + 2.0 * V * px * cout, 4.0 * (x + px * cout + w)};
}
// res: a ResKind, or RES_RAW0 for layer 0's residual conv on the data_bn'd keypoints ([rows][4])
constexpr int RES_RAW0 = 3;
inline Work tcn_work(double px_in, double px_out, int cin, int cout, int res) {
    Work w{2.0 * px_out * TK * cout * cout, 4.0 * (px_in * cout + px_out * cout + (double)TK * cout * cout)};
    if (res == RES_CONV || res == RES_RAW0) w.flops += 2.0 * px_out * cin * cout;
    if (res == RES_CONV) w.bytes += 4.0 * (px_out * cin + (double)cin * cout);
    if (res == RES_RAW0) w.bytes += 4.0 * px_out * 4;
    if (res == RES_IDEN) w.bytes += 4.0 * px_out * cout;
    return w;
}

// ---------------------------------------------------------------- debug hooks (debug.cpp)
extern thread_local Profiler* g_prof;   // set for the duration of a profiled call

// One annotated launch: the profiler's event pair around the scope and, with
// TIK_CHECKSUM=1, a checksum of its output buffer after it (tik_debug_checksums).
struct ProfScope {
    int i;
    hipStream_t st;
    const char* lab;
    const void* op = nullptr;
    size_t obytes = 0;
    void out(const void* p, size_t bytes) { op = p; obytes = bytes; }
    ProfScope(const char* label, Work w, hipStream_t s) : st(s), lab(label) {
        i = g_prof ? g_prof->begin(label, w.flops, w.bytes, s) : -1;
    }
    ~ProfScope();
};

// TIK_X_TRACE=1: the launch with per-workgroup phase stamps, its averages
// printed to stderr (scripts/xtrace.py); synchronizes the stream
hipError_t launch_xgemm_traced(tik::XArgs a, int bn, int epi, hipStream_t st, const char* label);
hipError_t launch_xgraph_traced(tik::XGraphArgs a, int ncu, hipStream_t st, const char* label);
hipError_t launch_xblock_traced(tik::XBlkArgs a, bool raw, int ncu, hipStream_t st, const char* label);

// ---------------------------------------------------------------- one StGcnBlock on the device
struct Layer;
// layer 0 from the raw keypoints (N,T,V,C0): data_bn inside its gcn kernel, the data_bn'd
// copy written to xb4 ([rows][4]) for the residual conv in the temporal conv's epilogue
struct RawInput {
    const float *kp, *bn_sc, *bn_sh;
    float* xb4;
};
// the next block's spatial half inside this block's xtws launch: its z goes to zn
struct FusedNext {
    const Layer* layer;
    float* zn;
};

struct Layer {
    int cin = 0, cinp = 0, cout = 0, stride = 1, res = RES_IDEN, V = 17, index = 0;
    bool mix_sparse = false;
    // cgemm.hip (fp32, and small batches): the folded fp32 weights of fold.h's FoldedBlock
    // and their bf16 planes p0+p1+p2
    DevBuf wg, bias2, amix, wt, wr, biasT;
    SplitW3 s3g, s3t, s3r;
    DevBuf wr0;             // layer0.hip / xblock.hip: [cout][cin] residual conv of a raw-input first layer
    DevHBuf xg, xt;         // xgemm.hip: bf16x3 tiles of the gcn (cin % 32 == 0) and of tcn (+ residual conv)
    int xg_bn = 0, xt_bn = 0, xt_ks = 0;
    DevHBuf xtw;            // xtws.hip: weight-stationary temporal conv (128 -> 128, stride 1, identity residual)
    DevHBuf xgw;            // xgraph.hip: weight-stationary gcn (128 / 256 output channels), planes in the MFMA register layout
    DevHBuf xbg, xbt;       // xblock.hip: whole block (64 channels, stride 1), gcn / tcn planes in the MFMA register layout
    int xgwon = 1;          // gcn on xgraph.hip where packed (TIK_XGW bit mask of layers; 0 = the XG tiles)
    int xtwson = 1;         // temporal conv on xtws.hip where packed (TIK_XTWS bit mask of layers; 0 = XT128)
    int xfgon = 1;          // the next block's gcn inside this block's xtws launch where possible (TIK_XFG bit mask)
    float* xtrash = nullptr;   // store target of rows past M (persistent kernels), owned by the model

    int pack(const FoldedBlock& f);   // upload, one block per kernel family (model.cpp)

    static int tout(int tin, int s) { return (tin - 1) / s + 1; }   // kt=3, pad=1

    // ---- which kernel family runs what
    bool x_ok() const { return xt.p && (xg.p || (index == 0 && wr0.p)); }   // the bf16x3 path covers this layer
    // the gcn runs on xgraph.hip
    bool xgw_path() const { return xgwon && xgw.p; }
    // the temporal conv runs on xtws.hip (input rows x of ld floats, tin frames per window)
    bool xtws_path(bool raw, int ld, int tin) const {
        return xtwson && xtw.p && !raw && res == RES_IDEN && stride == 1 && ld >= cout && ld % 4 == 0 && tin % 8 == 0;
    }
    // block `nx`'s spatial half can run inside this block's xtws launch (xtws.hip FG:
    // 128 -> 128 gcn planes on xgraph.hip's layout; TIK_XFG bit mask of this layer)
    bool fuses_gcn_of(const Layer& nx) const {
        return xfgon && xtw.p && nx.xgw_path() && nx.cin == cout && cout == 128 && nx.cout == 128;
    }
    // the 64-column temporal convs (6 K steps per tile) on the persistent xgemm kernel: it
    // hides the first-DMA prologue that is a large share of such short tiles
    bool xpt_path() const { return xt_bn == 64 && cout % xt_bn == 0; }

    // ---- launches (forward.cpp). x: fp32 rows [N*tin*V][ld] (ld >= cinp, % 4);
    // z: workspace N*tin*V*cout; out: [N*tout*V][cout]
    int forward(const float* x, int ld, int N, int tin, float* z, float* out, hipStream_t st, int prec,
                float* part = nullptr) const;                                        // cgemm.hip, both halves
    int spatial_x(const float* x, int ld, int N, int tin, float* z, hipStream_t st, int ncu,
                  const RawInput* raw) const;                                        // bf16x3: gcn -> z
    int temporal_x(const float* x, int ld, int N, int tin, const float* z, float* out, hipStream_t st, int ncu,
                   const RawInput* raw, const FusedNext* fg) const;                  // bf16x3: z -> out
};

}  // namespace tik_host

// ----------------------------------------------------------------------------
struct tik_model {
    int V = 17, C0 = 3, feat = 0, hidden = 0, pose_dim = 0;
    std::vector<tik_host::Layer> layers;
    tik_host::DevBuf bn_sc, bn_sh;           // data_bn (V*C0)
    tik_host::DevBuf w0, b0, w3, b3;         // head
    tik_host::SplitW3 s30, s33;
    tik_host::DevHBuf xh0;                   // bf16x3 tiles of pose_regressor.0 for xgemm.hip (feat % 32 == 0)
    static constexpr int XHEAD_KS = 4;       // xgemm head: K slices, fixed so a window's poses do not depend on the batch size
    int prec = 2;
    // ws[0]: the handle's workspace; ws[1] + a private stream: large batches run
    // as two parts on two streams, so one part's HBM-bound launches run beside
    // the other's MFMA-bound ones. Online-IK streams own their workspaces (stream.cpp).
    static constexpr int MAXSPLIT = 2;
    tik_host::Workspace ws[MAXSPLIT];
    hipStream_t aux[MAXSPLIT - 1] = {};
    hipEvent_t ev_fork = nullptr, ev_join[MAXSPLIT - 1] = {};
    bool split = true;                 // TIK_SPLIT=0: one stream
    std::atomic<int> refs{1};          // the handle + every live online-IK stream
    ~tik_model() {
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        for (auto e : ev_join) if (e) (void)hipEventDestroy(e);
        for (auto a : aux) if (a) (void)hipStreamDestroy(a);
    }
    int x_chunk_max = 0;               // test hook (TIK_X_CHUNK): cap on windows per sub-batch
    bool xblk = true;                  // blocks 0 and 1 as whole-block kernels (xblock.hip; TIK_XBLK=0: layered G + T)
    int ncu = 256;                     // compute units (persistent grids)
    tik_host::DevHBuf trash;           // scratch line for the persistent kernels' stores of invalid rows
    tik_host::Profiler prof;
    bool profiling = false;

    // the backbone runs on the bf16x3 kernels (xgemm.hip and its kin); else cgemm.hip
    bool use_x() const {
        if (prec != tik::PREC_BF16X3) return false;
        for (const auto& L : layers)
            if (!L.x_ok() || (L.index == 0) != (L.cin <= 4)) return false;
        return true;
    }
    // ... with blocks 0 and 1 as whole-block kernels (xblock.hip)
    bool use_xblk() const {
        if (!xblk || layers.size() < 2) return false;
        const auto &L0 = layers[0], &L1 = layers[1];
        return L0.cout == 64 && L0.stride == 1 && L0.res == tik_host::RES_CONV && L0.wr0.p && L0.xbt.p &&
               L1.cin == 64 && L1.cout == 64 && L1.stride == 1 && L1.res == tik_host::RES_IDEN && L1.xbt.p && L1.xbg.p;
    }
};

struct tik_block {
    tik_host::Layer layer;
    tik_host::DevBuf xp, z;   // padded-input and z workspace
    int prec = 2;
};

namespace tik_host {
struct ProfGuard {   // a call on a profiling handle: its launches go to the handle's profiler
    ProfGuard(tik_model* m) { g_prof = (m && m->profiling) ? &m->prof : nullptr; }
    ~ProfGuard() { g_prof = nullptr; }
};

// Bytes per pixel (frame x joint) of block 0's output when blocks 0 and 1 run
// whole (xblock.hip): 64 channels as three bf16 planes, written into the z
// workspace (blocks01_x), so z must hold N*T*V of them whatever the widths of
// the later layers.
constexpr size_t XB0_P3_FLOATS = 64 * 3 * 2 / 4;
}  // namespace tik_host
