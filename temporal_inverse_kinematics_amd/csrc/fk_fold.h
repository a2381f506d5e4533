// fk_fold.h — the host side of an SMPL-X constant set, with no HIP call in it:
// validation of the tensors tik_fk_create is given, and everything it uploads.
//
//   PT   [3V][KP]   row 3v+c = [posedirs[:,3v+c] | shapedirs[v,c,:] | exprdirs[v,c,:] | v_template[v,c] | 0..]
//   WT   [V][KJ]    lbs_weights, rows padded to KJ
//   jt, jd          J_regressor folded into the template and the blend shapes (float64 sums)
//   nzw  [V][nz]    per vertex the joints with W > 2^-30 as {joint, weight bits}, joints ascending
//   pick_v, pick_w  per joint >= 55 its (vertex, barycentric weight) picks; dyn_v the contour's by bin
//   anc  [55]       bit j of anc[k] = joint j is k or an ancestor of k
//
// Every tensor is checked for rank and for the number of values it really holds
// before any shape[i] or v[i] of it is read (include/tik.h is a C ABI: the
// tensors come from outside the program). Everything here runs before the first
// device allocation (fk_model.cpp), and stands alone in tests/test_fk_fold_host.py.
#pragma once
#include <algorithm>
#include <climits>
#include <cstring>

#include "fold.h"

namespace tik_host {

constexpr int NJ = 55;    // joints of the kinematic chain
constexpr int KP = 512;   // padded blend-shape K (486 pose + 20 shape + 1 template)
constexpr int KJ = 64;    // padded skinning K (55 joints)

struct FoldedSmplx {
    int V = 0, F = 0, nb = 0, ne = 0, nlmk = 0, ndyn = 0, nextra = 0, njoints = 0, nchain = 0, maxdepth = 0;
    int ldv = 0;   // v_posed row stride (3V rounded up to 4 floats: vector stores)
    int nz = 0;    // nzw entries per vertex: 4, 8 or 16; 0: a vertex has more than 16 live joints (the dense GEMM)
    bool contour = false;
    std::vector<float> PT, WT, jt, jd, pose_mean, lmk_bary, dyn_bary, pick_w;
    std::vector<int> parents, chain, faces, lmk_faces, dyn_faces, extra, depth, nzw, pick_v, dyn_v;
    std::vector<unsigned long long> anc;
};

inline const HostTensor* need(const TensorMap& m, const char* k, int& rc) {
    const HostTensor* t = find(m, k);
    if (!t) rc = fail(TIK_E_MISSING, "missing SMPL-X tensor '%s'", k);
    return t;
}

inline std::vector<int> to_int(const HostTensor* t) {
    std::vector<int> o(t->v.size());
    for (size_t i = 0; i < o.size(); ++i) o[i] = (int)std::lround(t->v[i]);
    return o;
}

// flags bit 0: the 17 dynamic contour landmarks, when both contour tables are given
inline int fold_smplx(const TensorMap& m, int flags, FoldedSmplx& f) {
    int rc = TIK_OK;
    const HostTensor* vt = need(m, "v_template", rc);
    const HostTensor* sd = need(m, "shapedirs", rc);
    const HostTensor* pd = need(m, "posedirs", rc);
    const HostTensor* jr = need(m, "J_regressor", rc);
    const HostTensor* lw = need(m, "lbs_weights", rc);
    const HostTensor* par = need(m, "parents", rc);
    const HostTensor* fc = need(m, "faces", rc);
    const HostTensor* lf = need(m, "lmk_faces_idx", rc);
    const HostTensor* lb = need(m, "lmk_bary_coords", rc);
    const HostTensor* ex = need(m, "extra_verts", rc);
    if (rc) return rc;
    const HostTensor* ed = find(m, "exprdirs");
    const HostTensor* pm = find(m, "pose_mean");
    const HostTensor* df = find(m, "dynamic_lmk_faces_idx");
    const HostTensor* db = find(m, "dynamic_lmk_bary_coords");
    auto bad = [](const char* msg) { return fail(TIK_E_INVALID, "tik_fk_create: %s", msg); };

    // ---- shapes and value counts, tensor by tensor
    if (vt->shape.size() != 2 || vt->shape[1] != 3 || vt->shape[0] > INT_MAX / (3 * KP)) return bad("v_template must be (V,3)");
    const int V = f.V = (int)vt->shape[0];
    if ((rc = expect(*vt, "v_template", 2, (size_t)V * 3))) return rc;
    if (sd->shape.size() != 3 || sd->shape[0] != V || sd->shape[1] != 3) return bad("shapedirs must be (V,3,nb)");
    if (ed && (ed->shape.size() != 3 || ed->shape[0] != V || ed->shape[1] != 3)) return bad("exprdirs must be (V,3,ne)");
    const int64_t NS64 = sd->shape[2] + (ed ? ed->shape[2] : 0);
    if (54 * 9 + NS64 + 1 > KP || NS64 > 32) return bad("too many shape components");
    f.nb = (int)sd->shape[2];
    f.ne = ed ? (int)ed->shape[2] : 0;
    const int NS = f.nb + f.ne;
    if ((rc = expect(*sd, "shapedirs", 3, (size_t)V * 3 * f.nb)) || (ed && (rc = expect(*ed, "exprdirs", 3, (size_t)V * 3 * f.ne))))
        return rc;
    if (pd->shape.size() != 2 || pd->shape[0] != 54 * 9 || pd->shape[1] != 3 * V) return bad("posedirs must be (486, 3V)");
    if ((rc = expect(*pd, "posedirs", 2, (size_t)486 * 3 * V))) return rc;
    if (jr->shape.size() != 2 || jr->shape[0] != NJ || jr->shape[1] != V) return bad("J_regressor must be (55,V)");
    if ((rc = expect(*jr, "J_regressor", 2, (size_t)NJ * V))) return rc;
    if (lw->shape.size() != 2 || lw->shape[0] != V || lw->shape[1] != NJ) return bad("lbs_weights must be (V,55)");
    if ((rc = expect(*lw, "lbs_weights", 2, (size_t)V * NJ))) return rc;
    if ((int)par->v.size() != NJ) return bad("parents must have 55 entries");
    if (fc->shape.size() != 2 || fc->shape[1] != 3 || fc->shape[0] > INT_MAX / 3) return bad("faces must be (F,3)");
    f.F = (int)fc->shape[0];
    if ((rc = expect(*fc, "faces", 2, (size_t)f.F * 3))) return rc;
    f.nlmk = (int)lf->v.size();
    f.nextra = (int)ex->v.size();
    if ((int)lb->v.size() != 3 * f.nlmk) return bad("lmk_bary_coords must be (L,3)");
    f.contour = (flags & 1) && df && db;
    if (f.contour && (df->shape.size() != 2 || df->shape[0] != 79 || df->shape[1] > INT_MAX / (79 * 3) ||
                      (int64_t)db->v.size() != 79 * df->shape[1] * 3))
        return bad("dynamic_lmk_faces_idx must be (79,D), dynamic_lmk_bary_coords (79,D,3)");
    f.ndyn = f.contour ? (int)df->shape[1] : 0;
    if (f.contour && (rc = expect(*df, "dynamic_lmk_faces_idx", 2, (size_t)79 * f.ndyn))) return rc;
    f.njoints = NJ + f.nextra + f.nlmk + f.ndyn;
    if (pm && (int)pm->v.size() != NJ * 3) return bad("pose_mean must be (55,3)");

    // ---- index tables
    f.parents = to_int(par); f.faces = to_int(fc); f.lmk_faces = to_int(lf); f.extra = to_int(ex);
    const std::vector<int> &hpar = f.parents, &hfaces = f.faces, &hlf = f.lmk_faces, &hex = f.extra;
    for (int j = 0; j < NJ; ++j)
        if (hpar[j] >= j || (j > 0 && hpar[j] < 0) || (j == 0 && hpar[j] != -1)) return bad("parents must be a topologically ordered tree rooted at 0");
    for (int i : hfaces) if (i < 0 || i >= V) return bad("face vertex index out of range ('faces')");
    for (int i : hlf) if (i < 0 || i >= f.F) return bad("landmark face index out of range ('lmk_faces_idx')");
    for (int v : hex) if (v < 0 || v >= V) return bad("extra vertex index out of range ('extra_verts')");
    f.dyn_faces.clear();
    if (f.contour) {
        f.dyn_faces = to_int(df);
        for (int i : f.dyn_faces) if (i < 0 || i >= f.F) return bad("dynamic landmark face index out of range ('dynamic_lmk_faces_idx')");
    }
    const std::vector<int>& hdf = f.dyn_faces;

    // ---- nothing below can refuse
    // depth of each joint in the tree: the chain kernel composes one level at a time
    f.depth.assign(NJ, 0);
    for (int j = 1; j < NJ; ++j) f.depth[j] = f.depth[hpar[j]] + 1;
    f.maxdepth = *std::max_element(f.depth.begin(), f.depth.end());
    f.ldv = (3 * V + 3) & ~3;
    // neck kinematic chain (smplx: from NECK_IDX=12 up to the root)
    f.chain.clear();
    for (int i = 12; i != -1; i = hpar[i]) f.chain.push_back(i);
    f.nchain = (int)f.chain.size();

    // blend-shape matrix P^T (3V, KP): row 3v+c = [posedirs[:,3v+c] | shapedirs[v,c,:] | exprdirs[v,c,:] | v_template[v,c] | 0]
    f.PT.assign((size_t)3 * V * KP, 0.f);
    for (int v = 0; v < V; ++v)
        for (int c = 0; c < 3; ++c) {
            float* row = &f.PT[(size_t)(3 * v + c) * KP];
            for (int p = 0; p < 486; ++p) row[p] = pd->v[(size_t)p * 3 * V + 3 * v + c];
            for (int l = 0; l < f.nb; ++l) row[486 + l] = sd->v[((size_t)v * 3 + c) * f.nb + l];
            for (int l = 0; l < f.ne; ++l) row[486 + f.nb + l] = ed->v[((size_t)v * 3 + c) * f.ne + l];
            row[486 + NS] = vt->v[(size_t)v * 3 + c];
        }
    f.WT.assign((size_t)V * KJ, 0.f);
    for (int v = 0; v < V; ++v)
        for (int j = 0; j < NJ; ++j) f.WT[(size_t)v * KJ + j] = lw->v[(size_t)v * NJ + j];
    // J_regressor folded into the template and blend shapes (float64 on the host)
    f.jt.resize(NJ * 3);
    f.jd.resize((size_t)NJ * 3 * NS);
    for (int j = 0; j < NJ; ++j)
        for (int c = 0; c < 3; ++c) {
            double s = 0.0;
            std::vector<double> d(NS, 0.0);
            for (int v = 0; v < V; ++v) {
                const double w = jr->v[(size_t)j * V + v];
                if (w == 0.0) continue;
                s += w * vt->v[(size_t)v * 3 + c];
                for (int l = 0; l < f.nb; ++l) d[l] += w * sd->v[((size_t)v * 3 + c) * f.nb + l];
                for (int l = 0; l < f.ne; ++l) d[f.nb + l] += w * ed->v[((size_t)v * 3 + c) * f.ne + l];
            }
            f.jt[j * 3 + c] = (float)s;
            for (int l = 0; l < NS; ++l) f.jd[((size_t)j * 3 + c) * NS + l] = (float)d[l];
        }
    f.pose_mean.assign(NJ * 3, 0.f);
    if (pm) f.pose_mean = pm->v;
    f.lmk_bary = lb->v;
    f.dyn_bary.clear();
    if (f.contour) f.dyn_bary = db->v;
    {   // sparse skinning weights
        const float tau = std::ldexp(1.0f, -30);
        int nzmax = 0;
        for (int v = 0; v < V; ++v) {
            int n = 0;
            for (int j = 0; j < NJ; ++j) n += lw->v[(size_t)v * NJ + j] > tau ? 1 : 0;
            nzmax = std::max(nzmax, n);
        }
        const int nz = f.nz = nzmax <= 4 ? 4 : nzmax <= 8 ? 8 : nzmax <= 16 ? 16 : 0;
        f.nzw.assign((size_t)V * nz * 2, 0);
        for (int v = 0; v < V && nz; ++v) {
            int n = 0;
            for (int j = 0; j < NJ; ++j) {
                const float w = lw->v[(size_t)v * NJ + j];
                if (w > tau) {
                    f.nzw[((size_t)v * nz + n) * 2] = j;
                    std::memcpy(&f.nzw[((size_t)v * nz + n) * 2 + 1], &w, 4);
                    ++n;
                }
            }
        }
    }
    {   // pick tables of the mesh-free joints path: vertex joints one pick of weight 1, landmarks three
        const int ns = f.nextra + f.nlmk;
        f.pick_v.assign((size_t)ns * 3, 0);
        f.pick_w.assign((size_t)ns * 3, 0.f);
        for (int k = 0; k < f.nextra; ++k) {
            f.pick_v[3 * k] = hex[k];
            f.pick_w[3 * k] = 1.0f;
        }
        for (int l = 0; l < f.nlmk; ++l)
            for (int i = 0; i < 3; ++i) {
                f.pick_v[3 * (f.nextra + l) + i] = hfaces[3 * hlf[l] + i];
                f.pick_w[3 * (f.nextra + l) + i] = lb->v[3 * l + i];
            }
        f.dyn_v.assign(hdf.size() * 3, 0);
        for (size_t e = 0; e < hdf.size(); ++e)
            for (int i = 0; i < 3; ++i) f.dyn_v[3 * e + i] = hfaces[3 * hdf[e] + i];
    }
    // ancestor-or-self masks of the Jacobian path (parents are topologically ordered)
    f.anc.assign(NJ, 0ull);
    for (int k = 0; k < NJ; ++k) f.anc[k] = (1ull << k) | (hpar[k] >= 0 ? f.anc[hpar[k]] : 0ull);
    return TIK_OK;
}

}  // namespace tik_host
