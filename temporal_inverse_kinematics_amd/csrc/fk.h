#pragma once
#include <hip/hip_runtime.h>

namespace tik {

struct FkChainArgs {
    int B, nb, ne, kp, kj, njoints, nchain;
    const float* pose;       // (B,55,3)
    const float* betas;      // (B,nb) or null
    const float* expr;       // (B,ne) or null
    const float* transl;     // (B,3) or null
    const float* pose_mean;  // (55,3)
    const int* parents;      // (55)
    const int* chain;        // neck kinematic chain (nchain)
    const float* jt;         // (55,3)        J_regressor . v_template
    const float* jd;         // (55,3,nb+ne)  J_regressor . [shapedirs | exprdirs]
    float* feat;             // (B,kp)  [vec(R_j - I), j=1..54 | betas | expr | 1 | 0..]  (fp32 GEMM path; or null)
    float* ablk;             // (B,arows,kj) rows e = 4r+c of A_j (3x4), cols j                (fp32 GEMM path; or null)
    int arows;               // rows of ablk per body: 16 (rows 12..15 = [0 0 0 1]) or 12 (the 3x4 part only)
    float* ajt;              // (55,B,12) A_j joint-major for the sparse / fused skinning (or null)
    float* joints;           // (B,njoints,3): first 55 written here
    int* dyn_bin;            // (B) or null
    const int* depth;        // (55) depth of each joint in the kinematic tree (root 0)
    int maxdepth;
};

// LBS on the sparse skinning weights: T = sum over the (at most nz)
// joints of vertex v with W[v][j] > 2^-30, in ascending joint order, in fp32
// FMAs (the dense product's terms in its order, minus terms below 2^-30 of a
// transform); one thread per vertex, a run of bodies per workgroup.
struct FkSkinSpArgs {
    int B, V, nz;                    // nz: entries per vertex (4, 8 or 16)
    const float* ajt;                // A_j joint-major: body b, joint j at ajt[(j * ajt_ld + b) * 12]
    int ajt_ld;                      // bodies per joint row of ajt (>= B: a chunk of a larger batch)
    const int2* nzw;                 // (V,nz) {joint, float bits of W[v][joint]}, joints ascending; padding {0, 0}
    const float* vposed;             // (B, ldv) v_posed, 3V used
    int ldv;
    const float* transl;             // (B,3): a zero array when the caller has none
    float* verts;                    // (B, 3V)
    int ncu;
};
hipError_t launch_fk_skin_sparse(const FkSkinSpArgs& a, hipStream_t st);

struct FkLmkArgs {
    int B, V, njoints, nextra, nlmk, ndyn;
    const float* verts;      // (B,V,3) including transl
    const float* transl;     // (B,3) or null
    const int* extra;        // (nextra)
    const int* faces;        // (F,3)
    const int* lmk_faces;    // (nlmk)
    const float* lmk_bary;   // (nlmk,3)
    const int* dyn_faces;    // (79,ndyn)
    const float* dyn_bary;   // (79,ndyn,3)
    const int* dyn_bin;      // (B)
    float* joints;           // (B,njoints,3): rows 55.. written here
};

hipError_t launch_fk_chain(const FkChainArgs& a, hipStream_t st);
hipError_t launch_fk_landmarks(const FkLmkArgs& a, hipStream_t st);

// Selected joints without the mesh (fk_joints.hip), after fk_chain_kernel wrote
// feat, ajt, dyn_bin and the (B,55,3) chain joints. Output column s is joint
// sel[s] (or s itself when sel_all). A joint below 55 is copied from jchain; any
// other is 1 (vertex joint) or 3 (landmark) vertex evaluations in fp32 FMAs:
//   v_posed[c] = sum_k feat[b][k] PT[3v+c][k]
//   T = sum_j W[v][j] A_j(b)                             joints ascending (nzw entries, or all 55 of WT)
//   x = T[:3,:3] v_posed + T[:,3];  joint = sum_i bary_i x_i + transl
// one lane per body; fk_joints.hip states the order of every sum.
constexpr int FKJ_MAX_SEL = 256;
constexpr int FKJ_TB = 64;   // bodies per workgroup tile (lane = body)
constexpr int FK_KP = 512;   // feature row length (fk_fold.h KP; asserted in fk_forward.cpp)
constexpr int FK_SD0 = 486;  // first shape column of a P^T row
// What the three mesh-free kernels (fk_joints.hip, fk_jacobian.hip, fk_shape.hip) all take, and fk_dev.h works on.
// nextra: joints 55 .. 55 + nextra are one vertex, later ones three; nz: nzw entries per vertex (4, 8, 16) or 0 = dense WT
struct FkSelArgs {
    int B, n_sel, nextra, nz;
    const float* ajt;        // (55,B,12)
    const float* PT;         // [3V][512]: shapedirs[v][c][i] at row 3 v + c, column 486 + i
    const float* WT;         // [V][64]
    const int2* nzw;         // (V,nz) or null
    const int* pick_v;       // (nextra+nlmk, 3) vertex ids of the static joints 55.. (a vertex joint uses entry 0)
    const float* pick_w;     // (nextra+nlmk, 3) their barycentric weights (vertex joint: 1, 0, 0)
    unsigned short sel[FKJ_MAX_SEL];   // output column s is joint sel[s]
};
struct FkJointsArgs : FkSelArgs {   // n_sel: the output columns, all njoints of them when sel_all (sel unused)
    int nlmk, ndyn, sel_all;
    int split;               // set by the launcher: workgroup per column, wave = 64-k chunk (small launches)
    const float* feat;       // (B,512)
    const float* jchain;     // (B,55,3) chain joints, transl included
    const float* transl;     // (B,3) or null
    const int* dyn_v;        // (79, ndyn, 3) contour vertex ids by bin
    const float* dyn_w;      // (79, ndyn, 3)
    const int* dyn_bin;      // (B)
    float* out;              // (B, n_sel, 3)
};
hipError_t launch_fk_joints(const FkJointsArgs& a, hipStream_t st);

// Jacobian of selected joints with respect to the pose (fk_jacobian.hip), after
// fk_chain_kernel wrote feat, ajt and the chain joints. Two launches:
//   fk_jac_pre_kernel   per (body, dof joint j): dR_a = d R_j / d theta_a (a = 0..2, the derivative of
//                       rodrigues_smplx as written) and the world-frame angular velocity
//                       omega_a = axial(G_parent.R dR_a G_j.R^T), into jw
//   fk_jacobian_kernel  lane = body, wave = output column s; for every dof the 3x3 block
//                       d joint sel[s] / d theta_j, stored as three runs of 3 floats in the body's rows
// jw is dof-major so that lane = body reads are coalesced: value q of dof d of body b at
// jw[(d * FKJAC_PER_DOF + q) * B + b], q < 27 dR_a[m] (9 a + m), 27 <= q < 36 omega_a[c] (27 + 3 a + c).
constexpr int FKJAC_PER_DOF = 36;
constexpr int FKJAC_WS = 55 * FKJAC_PER_DOF;   // floats of jw per body (include/tik.h: 1337 + 1980)
struct FkJacArgs : FkSelArgs {
    int n_dof;
    const float* pose;       // (B,55,3)
    const float* pose_mean;  // (55,3)
    const int* parents;      // (55)
    const unsigned long long* anc;   // (55) bit j of anc[k]: j is k or an ancestor of k
    const float* feat;       // (B,512)
    const float* jchain;     // (B,55,3), transl included
    const float* transl;     // (B,3) or null
    float* jw;               // (n_dof, FKJAC_PER_DOF, B)
    float* jac;              // (B, 3 n_sel, 3 n_dof)
    unsigned char dof[56];
};
hipError_t launch_fk_jacobian(const FkJacArgs& a, hipStream_t st);

// Jacobian of selected joints with respect to the shape (fk_shape.hip), after fk_chain_kernel wrote
// ajt. For a fixed pose the joints are affine in the betas, so only the world rotations R_k (the 3x3
// part of A_k in ajt) and constants enter. Two launches:
//   fk_shape_pre_kernel       per (body, beta i): dP_k,i, the derivative of the 55 posed chain joints,
//                             joints ascending (a parent comes before its children), into sw
//   fk_shape_jacobian_kernel  lane = body, wave = output column s; the nb derivatives of joint sel[s],
//                             stored as three runs of nb floats in the body's rows
// sw is beta-major so that lane = body reads are coalesced: component c of joint k for beta i of body b
// at sw[((i * 55 + k) * 3 + c) * B + b].
constexpr int FKS_MAX_NB = 25;        // nb + ne <= 25 by the 512-wide feature row
constexpr int FKS_PER_BETA = 55 * 3;  // floats of sw per body and beta (include/tik.h: 1337 + 165 nb)
struct FkShapeArgs : FkSelArgs {
    int nb, ns;              // ns = nb + ne: row length of jd
    const int* parents;      // (55), parents[k] < k
    const float* jd;         // (55,3,ns)  J_regressor . [shapedirs | exprdirs]
    float* sw;               // (nb, 55, 3, B)
    float* jac;              // (B, 3 n_sel, nb)
};
hipError_t launch_fk_shape_jacobian(const FkShapeArgs& a, hipStream_t st);

}  // namespace tik
