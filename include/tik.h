/*
 * tik.h — C ABI of libtik.so, the MI355X-native temporal-IK engine.
 *
 * Every compute entry point takes caller-owned DEVICE pointers (fp32,
 * row-major, explicit dims) and a hipStream_t passed as `void*` (NULL = the
 * legacy default stream), is stream-ordered, and returns an int status:
 * TIK_OK (0) or a negative TIK_E_* code; tik_last_error() returns the text of
 * the calling thread's last failure. Handles own their device weights and
 * workspace; per-call functions allocate only through the handle. One
 * handle serves one stream at a time: calls on the same handle must be
 * stream-ordered (they share its workspace, which a call may grow). Distinct
 * handles are independent. An online-IK stream (tik_stream_*) owns its own
 * workspace and a reference on its model, so it may run concurrently with
 * batch calls on that model's handle, and outlives tik_model_destroy.
 *
 * Each entry point names the reference interface it replaces
 * (paths relative to the reference repository root).
 */
#ifndef TIK_H
#define TIK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TIK_OK 0
#define TIK_E_INVALID (-1)   /* bad argument / shape: Python raises ValueError  */
#define TIK_E_HIP (-2)       /* HIP runtime error: Python raises RuntimeError   */
#define TIK_E_MISSING (-3)   /* missing state-dict tensor: Python raises KeyError */
#define TIK_E_NOMEM (-4)     /* device allocation failed                        */

typedef struct tik_model* tik_model_t;
typedef struct tik_fk* tik_fk_t;

/* One named host fp32 tensor of a state dict (weight ABI = reference keys). */
typedef struct {
    const char* name;      /* e.g. "backbone.st_gcn_networks.3.tcn.2.weight" */
    const float* data;     /* host pointer, contiguous                        */
    int ndim;
    int64_t shape[4];
} tik_tensor;

const char* tik_last_error(void);
const char* tik_version(void);
// Debug: with TIK_GUARD=1 in the environment every library buffer carries
// 1 MiB guard zones; returns the number of written guard zones (description
// in tik_last_error(), guards re-armed), or < 0 on error.
int tik_debug_check_guards(void);
// Debug: with TIK_POISON=<two hex digits> in the environment (read at every
// allocation, so it may be set after the library is loaded) the payload of
// every new library buffer is filled with that byte before it is returned;
// with TIK_GUARD=1 as well the guard zones keep 0xA5. ff = NaN as fp32 and as
// bf16, -1 as int; 7f = 3.39e38 as fp32 and as bf16, finite, so it survives a
// `s > 0 ? s : 0` ReLU, which flushes NaN to 0. Any other spelling fails the
// allocation with TIK_E_INVALID. tik_debug_alloc_fill returns the fill byte
// of the most recent allocation, or -1 (none yet, or it was not filled).
int tik_debug_alloc_fill(void);
// Debug: with TIK_CHECKSUM set, every launch of the IK forward is followed by
// a synchronising checksum of its output; copies "label:hex;..." of the
// launches since the last call into buf and clears the record.
int tik_debug_checksums(char* buf, int len);

/* ------------------------------------------------------------------------
 * IK model: PoseRegressor = StgGcn18 backbone + MLP head.
 * Replaces pose_trainer.py:66-133 (PoseRegressor.__init__/forward) and
 * IKPoseTrainer.forward pose_trainer.py:143-144, as called by
 * inference.run_inference inference.py:51.
 *
 * tik_model_create: `tensors` is the PoseRegressor state dict (keys without
 * the Lightning "regressor." prefix; num_batches_tracked ignored). Layer
 * shapes are inferred from the tensors (pose_trainer.py:76-83 config).
 * BatchNorm (eval) is folded into the convolutions on the host, then the
 * packed weights are uploaded once.
 * ---------------------------------------------------------------------- */
int tik_model_create(const tik_tensor* tensors, int n_tensors, tik_model_t* out);
int tik_model_destroy(tik_model_t m);
/* Output frames T' for an input window of T frames (4 stride-2 layers). */
int tik_model_out_frames(tik_model_t m, int T);
/* Grow the handle-owned workspace for batches up to (N,T); optional. */
int tik_model_reserve(tik_model_t m, int N, int T);
/* keypoints x: (N,T,V=17,C=3) fp32 device; poses: (N,T',66) fp32 device. */
int tik_ik_forward(tik_model_t m, const float* x, int N, int T, float* poses, void* stream);
/* Backbone only (StgGcn18.forward, st_gcn_aaai18.py:113-133): feat (N,T',V*Cout).
 * A handle created from a backbone-only state dict (StgGcn18's own keys, no
 * head) serves this call only; tik_ik_forward and tik_stream_create refuse it. */
int tik_backbone_forward(tik_model_t m, const float* x, int N, int T, float* feat, void* stream);

/* GEMM arithmetic (both accumulate in fp32):
 * 0 = exact fp32 MFMA (v_mfma_f32_16x16x4_f32);
 * 2 = 6-product bf16 split (v_mfma_f32_16x16x32_bf16 on x = p0 + p1 + p2,
 *     products p_i q_j with i + j <= 2: fp32's exponent range, ~2^-24
 *     relative per product) — the DEFAULT.
 * (1, a 3-term f16 split with f16's narrower range, is retired: the setters
 * return TIK_E_INVALID for it.) The environment variable
 * TIK_PRECISION=fp32|bf16x3 picks the arithmetic at handle creation. */
#define TIK_PREC_F32 0
#define TIK_PREC_BF16X3 2
int tik_model_set_precision(tik_model_t m, int prec);
int tik_model_get_precision(tik_model_t m);

/* Per-launch HIP-event profiling of the model's kernels (used by bench.py):
 * tik_model_profile(m, n) records up to n launches (0 disables, clears);
 * after synchronising, tik_model_profile_read returns launch i's label
 * ("<tile config>.<role>"), elapsed ms, and algorithmic FLOPs / bytes. */
int tik_model_profile(tik_model_t m, int max_launches);
int tik_model_profile_count(tik_model_t m);
int tik_model_profile_read(tik_model_t m, int i, char* label, int label_len, float* ms, double* flops,
                           double* bytes);

/* ------------------------------------------------------------------------
 * One StGcnBlock (st_gcn_aaai18.py:136-214, eval mode) on channels-last data.
 * x: (N,T,V,Cin) device, out: (N,T',V,Cout) device, A_eff: (V,V) device
 * (= A * edge_importance, st_gcn_aaai18.py:129), K = 1 (uniform strategy).
 * `tensors` is the block's state dict (keys "gcn.conv.weight", "tcn.0.*",
 * "tcn.2.*", "tcn.3.*", "residual.0.*", "residual.1.*").
 * residual: 0 = none (zero), 1 = module default (iden or conv per :191-204).
 * ---------------------------------------------------------------------- */
typedef struct tik_block* tik_block_t;
int tik_block_create(const tik_tensor* tensors, int n_tensors, int in_channels, int out_channels,
                     int stride, int residual, const float* A_eff_host, int V, tik_block_t* out);
int tik_block_destroy(tik_block_t b);
int tik_stgcn_block_fwd(tik_block_t b, const float* x, int N, int T, float* out, void* stream);
int tik_block_set_precision(tik_block_t b, int prec);

/* ------------------------------------------------------------------------
 * ConvTemporalGraphical.forward (gconv_origin.py:56-65), reference layout.
 * x (N,Cin,T,V), A (K,V,V), W (K*Cout, Cin, t_kernel, 1), b (K*Cout) or NULL,
 * out (N,Cout,T_out,V) with T_out = (T + 2p - d*(tk-1) - 1)/s + 1. All device.
 * ---------------------------------------------------------------------- */
int tik_gconv_fwd(const float* x, int N, int Cin, int T, int V, const float* A, int K,
                  const float* W, const float* b, int Cout, int t_kernel, int t_stride,
                  int t_padding, int t_dilation, float* out, void* stream);

/* ------------------------------------------------------------------------
 * kornia angle_axis_to_rotation_matrix (common/kornia_geometry_conversion.py:125-201):
 * aa (n,3) -> R (n,3,3), device pointers.
 * ---------------------------------------------------------------------- */
int tik_aa_to_rotmat(const float* aa, int n, float* R, void* stream);

/* ------------------------------------------------------------------------
 * Windowing (mmskeleton/datasets/data_amass.py:18-42 sample_window and
 * :221-236 InferenceDataset, relative_pose=True) on the device:
 * seq (F,V,3) -> windows (n_idx, 2h+1, V, 3) for centre frames
 * idx0 .. idx0+n_idx-1, edge-padded, root-relative (root = mean of joints
 * root_a, root_b; COCO 11/12). Returns TIK_E_INVALID when any requested
 * window would raise ValueError or be short in the reference.
 * ---------------------------------------------------------------------- */
int tik_window_gather(const float* seq, int F, int V, int idx0, int n_idx, int h, int root_a,
                      int root_b, int relative, float* windows, void* stream);

/* ------------------------------------------------------------------------
 * moveai_3d -> COCO-17 keypoints on the device (inference.py:121-133 with
 * common/keypoints_util.py:27-60 generate_moveai3d_to_coco_mappings /
 * convert_seq_keypoints): out[f][c] = joints[f][map17[c]] (map17: 17 host ints,
 * -1 = none), COCO 0 = 0.5 (joints[f][J-1] + joints[f][J-2]) (nose = mid of
 * the ears), 1 = joints[f][J-2], 2 = joints[f][J-1] (eyes = ears), then
 * (x, y, z) -> (x, z, -y). joints (F,J,3), out (F,17,3), device fp32.
 * ---------------------------------------------------------------------- */
int tik_moveai_to_coco(const float* joints, int F, int J, const int* map17_host, float* out, void* stream);

/* ------------------------------------------------------------------------
 * Online IK (BASELINE.json config #5): stride-1 sliding window over a live
 * sequence. tik_stream_push copies one frame (V=17 x 3 host floats) into a
 * device ring, gathers the window centred h = win_size/2 frames back (left
 * edge clamped as data_amass.py:18-42), runs the IK forward (N=1) and returns
 * pose row 0 (66 floats) — identical to inference.run_inference's frame
 * (inference.py:37-67). Returns 1 when a pose was produced (after h+1 pushes),
 * 0 before, <0 on error. The step is one hipGraph replay when use_graph != 0.
 * Flush the last h frames by pushing the last frame h more times.
 * A frame with a NaN or an Inf in it is refused: tik_stream_push checks the 51
 * floats on the host before anything is copied or enqueued and returns
 * TIK_E_INVALID (tik_last_error names the index of the first such value). The
 * frame is not appended: ring, frame count and the pose of every other frame
 * are those of a stream that was never offered it. (The dataflow kernel's
 * ReLUs turn a NaN into 0, so such a frame would otherwise give finite, wrong
 * poses for every window that holds it.)
 * ---------------------------------------------------------------------- */
/* The stream keeps a reference on `model` (released by tik_stream_destroy)
 * and private buffers for the one step it runs (tik_stream_path): batch calls
 * on the model handle (any size, any stream) do not disturb a live stream.
 * tik_stream_create refuses (TIK_E_INVALID, before any device call) a
 * win_size that is not positive or so large that 2 (2h+1) exceeds 2^29, a
 * backbone-only handle, and a model whose pose width (rows of
 * pose_regressor.3) is not 66. */
typedef struct tik_stream* tik_stream_t;
int tik_stream_create(tik_model_t model, int win_size, int use_graph, tik_stream_t* out);
int tik_stream_destroy(tik_stream_t s);
int tik_stream_reset(tik_stream_t s);
int tik_stream_push(tik_stream_t s, const float* frame_host, float* pose_host);
/* Which step the stream runs: 1 = the single dataflow kernel (online.hip:
 * only the frames pose row 0 depends on, fp32, frame read from and pose
 * written to pinned host memory by the kernel; TIK_ONLINE=0 disables it),
 * 0 = the layered IK forward on the whole window (models it cannot run). */
int tik_stream_path(tik_stream_t s);
/* Refinement inside the stream: after the IK step, one more launch of
 * tik_fk_refine's kernel (B = 1, COCO-17 on SMPL-X, see there) refines the pose
 * the step just solved against the keypoints of its own frame c = count - 1 - h,
 * read from the device ring. prior = the network's pose; with smooth > 0 the
 * cost also ties the pose to the previous *refined* pose, the causal
 * counterpart of tik_lm_solve_chain's smoothness (none for frame 0 and after
 * tik_stream_reset). It is a separate launch in stream order on the stream's
 * one private stream: the captured graph stays a linear chain, and
 * tik_stream_set_refine records it again. The kernel writes the refined pose
 * and then a done word to pinned host memory; tik_stream_push waits on that word
 * and returns the refined pose. While the stream is still filling (c < 0) the
 * pose passes through unrefined. betas_host: tik_fk's nb values or NULL (the
 * mean shape); joint_w_host: 17 non-negative keypoint weights or NULL (ones);
 * both are copied. The stream keeps a reference on `fk` (released when
 * refinement is switched off or the stream destroyed). iters = 0 switches
 * refinement off (fk and the rest are ignored). Call it between pushes.
 * TIK_E_INVALID, leaving the stream as it was: iters < 0, mu <= 0, smooth < 0,
 * lam0 <= 0, a negative weight, a NULL fk, a body model whose COCO-17 joints
 * the kernel does not take.
 * tik_stream_raw_pose: the network's own pose of the last push that returned
 * one (what that push would have returned without refinement), 66 floats. */
int tik_stream_set_refine(tik_stream_t s, tik_fk_t fk, const float* betas_host, const float* joint_w_host,
                          int iters, float mu, float smooth, float lam0);
int tik_stream_raw_pose(tik_stream_t s, float* pose_host);
/* Imperfect detections. tik_stream_push_conf is tik_stream_push with 17
 * confidences (host, >= 0). Keypoint k is missing when conf[k] is 0 or one of
 * its coordinates is NaN or Inf (a non-finite keypoint with positive
 * confidence counts as confidence 0). The fill runs on the host before the
 * frame goes to pinned memory: a missing keypoint takes the last value this
 * stream accepted for it, in absolute coordinates (hold-last; a stated rule,
 * not a tuned one: nobody has measured it on real detections), so the ring
 * never holds a non-finite value and the network sees a complete frame.
 * TIK_E_INVALID, the frame not appended and the stream as if never offered it:
 * a missing keypoint not seen since create or tik_stream_reset (which clears
 * the last-seen state), a confidence that is negative, NaN or infinite.
 * A refining stream keeps W x 17 confidences beside the keypoint ring: the
 * refine launch reads this push's 17 from pinned host memory, stores them at
 * the slot of frame count - 1 and refines frame c = count - 1 - h with
 * keypoint weights conf_c[k] * joint_w[k] (one fp32 multiply); if conf_c[11]
 * or conf_c[12] is 0 all 17 are 0 and the pose moves only toward the network's
 * and the previous refined pose. tik_stream_push on such a stream is the push
 * with confidences of one, and gives the bits it gave before. A stream without
 * refinement takes tik_stream_push_conf too: the fill only.
 * tik_stream_set_robust: the robust scale (tik_fk_refine_robust's
 * robust_sigma) of the refine launch, 0 = off; records the step again like
 * tik_stream_set_refine, which keeps the scale. Call it between pushes.
 * TIK_E_INVALID: sigma negative, NaN or infinite. */
int tik_stream_push_conf(tik_stream_t s, const float* frame_host, const float* conf_host, float* pose_host);
int tik_stream_set_robust(tik_stream_t s, float sigma);
/* Debug (TIK_ONLINE_TRACE=1 at create): the last step's per-task timestamps
 * {ticket taken, inputs ready, staged, computed, reduced, stores complete,
 * done, workgroup} (s_memrealtime ticks, 100 MHz; staged .. reduced: gcn and
 * temporal-conv tasks only)
 * in task order; returns the task count. */
int tik_debug_stream_trace(tik_stream_t s, long long* out, int cap);
/* Test hook: mark the dataflow kernel's dependency-timeout flag, as a real
 * 0.5 s wait timeout would; the next tik_stream_push then fails (that frame's
 * pose is invalid, the frame is still appended) and the one after it works. */
int tik_debug_stream_inject_error(tik_stream_t s);
/* Test hook: move the stream's frame count to `count`, which must be congruent to
 * the current count modulo 2 * (2h + 1) (the same ring slot and launch parity),
 * e.g. to just below the 2^30 wrap of stream_next_count (csrc/online.h). */
int tik_debug_stream_set_count(tik_stream_t s, int count);

/* ------------------------------------------------------------------------
 * Training-data generation (data half): AmassDataset
 * (mmskeleton/datasets/data_amass.py:87-218) on the GPU.
 * tik_rotate_root_z: regenerate_data's root-orientation augmentation
 * (:184-190) in place on pose rows (ld floats, first 3 = root axis-angle):
 * rotvec(R_z(angle) R(root)), float64 as scipy's Rotation does it.
 * tik_train_windows: __getitem__ (:125-154) for B items: edge-padded window
 * (2h+1 frames, h <= 64) of the FK joints [rows][n_joints][3] -> COCO-17
 * (coco_map, host) -> root-relative -> per-joint Gaussian noise (sigma, host:
 * coco_kps_sigma) -> windows [B][2h+1][17][3]; target = pose row of the
 * window's last frame, first 66 values -> [B][66]. Items (device int arrays):
 * sequence start row, sequence length, window centre, dataset index (the
 * noise stream: counter-based, keyed by (seed, index)). The caller checks the
 * reference's ValueError / short-window cases (the Python layer does).
 * ---------------------------------------------------------------------- */
int tik_rotate_root_z(float* poses, int F, int ld, double angle, void* stream);
int tik_train_windows(const float* joints, int n_joints, const float* poses, int pose_ld, const int* item_start,
                      const int* item_len, const int* item_idx, const int* item_uid, int B, int h,
                      const int* coco_map, const float* sigma, int relative, int add_noise, unsigned long long seed,
                      float* windows, float* target, void* stream);

/* ------------------------------------------------------------------------
 * Training step (optimizer half). Replaces
 * IKPoseTrainer.training_step (pose_trainer.py:146-155) as Lightning runs it:
 * train-mode forward (batch-statistics BatchNorm with the running-stat
 * update, Dropout(0.7) in the head, pose_trainer.py:89-92), nn.MSELoss
 * against the target poses (PoseLosses, :42-50), backward, and one
 * torch.optim.Adam(lr) update (configure_optimizers, :196-197).
 *
 * tik_trainer_create: the PoseRegressor state dict (as tik_model_create,
 *   incl. "tik.strides"); parameters and buffers are copied to the device.
 *   Every tensor is checked for rank and for the exact number of values it
 *   holds: a malformed one (wrong rank, null data, short or long, an empty
 *   or fractional "tik.strides") is refused by name, TIK_E_INVALID, before
 *   any device call.
 * tik_trainer_step: x [N][T][17][3], target [N][T'][66] (device fp32);
 *   dropout_mask [N*T'][512] of 0/1 (device), or NULL = a counter-based mask
 *   keyed by `seed`; loss: device float (or NULL). Stream-ordered.
 * tik_trainer_count / _tensor / _read: the state dict after the last step,
 *   in the reference's names and layouts (kind 0 = parameter, 1 = buffer);
 *   what = 0 value, 1 last gradient, 2 Adam exp_avg, 3 Adam exp_avg_sq,
 *   copied to a device pointer. tik_trainer_steps: updates taken
 *   (BatchNorm num_batches_tracked).
 * ---------------------------------------------------------------------- */
typedef struct tik_trainer* tik_trainer_t;
int tik_trainer_create(const tik_tensor* tensors, int n_tensors, float lr, tik_trainer_t* out);
int tik_trainer_destroy(tik_trainer_t t);
int tik_trainer_step(tik_trainer_t t, const float* x, int N, int T, const float* target, const float* dropout_mask,
                     unsigned long long seed, float* loss, void* stream);
int tik_trainer_out_frames(tik_trainer_t t, int T);
int tik_trainer_count(tik_trainer_t t);
int tik_trainer_tensor(tik_trainer_t t, int i, char* name, int name_len, int64_t* shape4, int* ndim, int* kind);
int tik_trainer_read(tik_trainer_t t, int i, int what, float* dst, void* stream);
long long tik_trainer_steps(tik_trainer_t t);
/* Validation and resume.
 * tik_trainer_eval: eval-mode forward on the trainer's current weights
 *   (BatchNorm on the running statistics, folded into the fp32 GEMM operands
 *   on the device; no dropout). poses (N,T',pose_dim) and loss (device scalar,
 *   mean((poses - target)^2)) are each optional; target is required iff
 *   loss != NULL. Changes no trainer state (parameters, gradients, Adam
 *   moments, running statistics, saved activations, steps). N*T == 1 is
 *   allowed (no batch statistics are taken), and a window's poses do not
 *   depend on the rest of the batch. Stream-ordered.
 * tik_trainer_write: the inverse of tik_trainer_read: device src -> value /
 *   gradient / exp_avg / exp_avg_sq of tensor i (buffers: what == 0 only).
 *   The derived GEMM layouts and the eval set are refreshed before their next
 *   use.
 * tik_trainer_set_steps: the update count (>= 0) that tik_trainer_steps
 *   reports and Adam's bias correction continues from (resuming a
 *   checkpoint; GpuTrainer also keys its dropout seed on it). */
int tik_trainer_eval(tik_trainer_t t, const float* x, int N, int T, const float* target, float* poses, float* loss,
                     void* stream);
int tik_trainer_write(tik_trainer_t t, int i, int what, const float* src, void* stream);
int tik_trainer_set_steps(tik_trainer_t t, long long steps);
/* Debug / test hook: the last step's saved activations of block `layer`
 * (which 0 output, 2 tcn conv output, 3 post-ReLU tcn input, 4 graph-mix
 * output, 5 gcn conv output; 6 the head's first Linear output), and with
 * TIK_TRAIN_DEBUG=1 (TIK_TRAIN_DEBUG_LAYER=l) its input gradient (1) and
 * backward intermediates (10..14); n floats to device dst. Both variables
 * are read by tik_trainer_create, which refuses a layer outside 0..L-1. */
int tik_trainer_debug(tik_trainer_t t, int which, int layer, float* dst, long long n, void* stream);
/* The head of the last step (any layer index in range): which 7 its train-mode
 * output (the predicted poses), 8 the loss gradient with respect to it, each
 * as (N T', pose_dim) dense; whole rows only, min(n / pose_dim, N T') of them. */

/* The training step with a keypoint term in the loss (tik_fk_keypoint_loss
 * below, back-propagated through FK), pose_dim 66. With R = N T' rows,
 *   kp_mse = (1 / (51 R)) sum_f sum_k w_k |r_fk|^2      (nn.MSELoss's normalisation of the 51 R residuals)
 *   loss   = pose_mse + weight kp_mse
 *   d loss / d poses[f] += weight (2 / (51 R)) J_f^T W r_f
 * After the MSE gradient is written, one tik_fk_keypoint_loss launch per body
 * model on its rows of the predicted poses (accumulate onto the gradient), then
 * one reduction of the per-frame losses (fixed order, in double); the head and
 * backbone backward and Adam follow unchanged. Rows that no list names count
 * as zero. rows[i]: device int32, distinct rows of the (R, .) pose matrix for
 * fk[i], n_rows[i] of them (0: no launch); no entry is range-checked on the
 * device, and a row in two lists is the caller's error. rows[0] == NULL with
 * n_models == 1: all R rows. kps (R,17,3), betas (R,nb) rows betas_ld apart
 * (betas_ld 0: one row for all) or NULL, joint_w 17 shared weights or NULL: device
 * fp32. loss: the total (device float, or NULL); loss_parts: {pose_mse, kp_mse}
 * (two device floats, or NULL). kp == NULL: exactly the launches of
 * tik_trainer_step (loss_parts must be NULL). weight == 0: kp_mse is still
 * reported (a monitor), and every gradient, Adam moment and parameter has the
 * bits of tik_trainer_step.
 * TIK_E_INVALID, before any kernel touches running statistics: what
 * tik_trainer_step refuses; a pose_dim other than 66; n_models outside 1..3; a
 * null fk[i]; a null rows[i] except the all-rows case; a negative n_rows[i] or
 * more than R rows in all; a null kps; a negative, NaN or infinite weight; what
 * tik_fk_keypoint_loss refuses of a model or of betas_ld. */
typedef struct {
    int n_models;              /* 1..3 body models (genders) in this batch */
    tik_fk_t fk[3];
    const int* rows[3];
    int n_rows[3];
    const float* kps;
    const float* betas;
    int betas_ld;
    const float* joint_w;
    float weight;              /* >= 0 */
} tik_kp_loss;
int tik_trainer_step_kp(tik_trainer_t t, const float* x, int N, int T, const float* target, const float* dropout_mask,
                        unsigned long long seed, const tik_kp_loss* kp, float* loss, float* loss_parts, void* stream);

/* ------------------------------------------------------------------------
 * SMPL-X forward kinematics + linear blend skinning (the FK check).
 * Replaces common/smpl_util.py:8-82 (load_smplx_models / run_smpl_inference)
 * and the third-party smplx.SMPLX.forward it calls (smpl_util.py:67-69;
 * create(model_type='smplx', use_pca=False, use_face_contour=True)).
 *
 * tik_fk_create: named host tensors (integer tables passed as exact floats):
 *   v_template (V,3), shapedirs (V,3,nb), [exprdirs (V,3,ne)], posedirs (486,3V),
 *   J_regressor (55,V), lbs_weights (V,55), parents (55), faces (F,3),
 *   lmk_faces_idx (L), lmk_bary_coords (L,3), extra_verts (21),
 *   [pose_mean (55,3)] (flat_hand_mean=False hand mean),
 *   [dynamic_lmk_faces_idx (79,D), dynamic_lmk_bary_coords (79,D,3)].
 * flags bit 0: use_face_contour (needs the dynamic tables).
 * tik_fk_forward: full_pose (B,55,3) [global, 21 body, jaw, leye, reye,
 *   15 lhand, 15 rhand], betas (B,nb)/NULL, expression (B,ne)/NULL,
 *   transl (B,3)/NULL -> joints (B, 55+21+L+D, 3), verts (B,V,3) or NULL.
 * ---------------------------------------------------------------------- */
int tik_fk_create(const tik_tensor* tensors, int n_tensors, int flags, tik_fk_t* out);
int tik_fk_destroy(tik_fk_t fk);
int tik_fk_set_precision(tik_fk_t fk, int prec);
int tik_fk_num_joints(tik_fk_t fk);
int tik_fk_num_verts(tik_fk_t fk);
int tik_fk_reserve(tik_fk_t fk, int B);
int tik_fk_forward(tik_fk_t fk, const float* full_pose, const float* betas, const float* expression,
                   const float* transl, int B, float* joints, float* verts, void* stream);
/* Joints of tik_fk_forward without the mesh. sel_host: n_sel joint indices in
 * [0, tik_fk_num_joints) in output order (duplicates allowed), or NULL = all
 * joints in order (n_sel ignored). out: (B, n_sel or njoints, 3) device fp32.
 * Joints below 55 are the chain's, bit for bit those of tik_fk_forward. Every
 * other joint is 1 or 3 vertices of the body, and only those are evaluated
 * (blend shapes, skinning, barycentric sum; vertices no selected joint needs
 * are skipped), in fp32 FMAs whose order is fixed: a body's joints are the
 * same bits for any B, any place in the batch and any selection.
 * tik_fk_set_precision does not change this path (fp32 FMAs in both settings;
 * within 2e-4 of tik_fk_forward's joints). The selection (at most 256
 * entries) travels in the kernel arguments: a call uploads nothing and is
 * stream-ordered like tik_fk_forward. Workspace: 1337 floats per body (pose
 * feature, transforms, chain joints); the mesh path's vertex buffers are never
 * reserved. TIK_E_INVALID: null pointers, B <= 0, an index out of range,
 * n_sel outside 1..256. */
int tik_fk_joints(tik_fk_t fk, const float* full_pose, const float* betas, const float* expression,
                  const float* transl, int B, const int* sel_host, int n_sel, float* out, void* stream);
/* Jacobian of selected joints with respect to the pose, without the mesh:
 * jac[b][3 s + c][3 d + a] = d joint sel[s] component c / d full_pose[b][dof[d]][a]
 * at the given inputs; jac is (B, 3 n_sel, 3 n_dof) device fp32, row-major.
 * sel_host: n_sel (1..256) joint indices as tik_fk_joints (NULL is not allowed
 * here): the 55 chain joints, the vertex joints and the static landmarks. A
 * contour landmark picks its vertices by a pose-dependent bin, so its selection
 * is piecewise constant: an index in that range is TIK_E_INVALID. dof_host:
 * n_dof (1..55) distinct pose joints in [0, 55), or NULL = joints 0..21 (n_dof
 * ignored). joints: (B, n_sel, 3) or NULL; when given it is written by
 * tik_fk_joints itself (the same bits). The derivative is that of the function
 * tik_fk_joints evaluates (rodrigues_smplx with its 1e-8 shift, pose_mean
 * added): entries of a chain joint for a dof that is not a strict ancestor of
 * it are exactly 0. fp32 FMAs in a fixed order for either tik_fk_set_precision
 * setting: a body's rows are the same bits for any B, any place in the batch
 * and any selection around a column. Selection and dof list travel in the kernel
 * arguments: a call uploads nothing and is stream-ordered. Workspace: 3317
 * floats per body (tik_fk_joints' 1337 + 1980: the rotation derivatives and
 * angular velocities of 55 dofs, 36 floats each; plus one int per body on a
 * handle with face contours); the mesh path's buffers are never reserved.
 * TIK_E_INVALID: null pointers, B <= 0, n_sel outside 1..256, a joint index out
 * of range or a contour landmark, n_dof outside 1..55, a dof index out of range
 * or repeated. */
int tik_fk_joints_jacobian(tik_fk_t fk, const float* full_pose, const float* betas, const float* expression,
                           const float* transl, int B, const int* sel_host, int n_sel, const int* dof_host, int n_dof,
                           float* jac, float* joints, void* stream);
/* Jacobian of selected joints with respect to the shape, without the mesh:
 * jac[b][3 s + c][i] = d joint sel[s] component c / d betas[b][i], i < nb =
 * shapedirs.shape[2]; jac is (B, 3 n_sel, nb) device fp32, row-major. For a
 * fixed pose the SMPL-X joints are affine in the betas, so this is the exact
 * difference joints(betas + e_i) - joints(betas), and it is a function of the
 * pose alone: betas, expression and transl (each may be NULL) are passed on to
 * tik_fk_joints when joints are asked for and do not change a bit of jac.
 * sel_host: n_sel (1..256) joint indices as tik_fk_joints_jacobian (NULL is not
 * allowed): the 55 chain joints, the vertex joints and the static landmarks. A
 * contour landmark's bin depends on the pose only, so it has a shape Jacobian,
 * but this call does not read the dynamic tables: an index in that range is
 * TIK_E_INVALID. joints: (B, n_sel, 3) or NULL; when given it is written by
 * tik_fk_joints itself (the same bits). With R_k the world rotation of chain
 * joint k, jd = J_regressor . shapedirs and sd_v = shapedirs[v]:
 *   chain joint k:  dP_k = dP_parent + R_parent (jd[k] - jd[parent]),  dP_0 = jd[0]
 *   vertex v:       sum over its skinning entries of W[v][k] (R_k (sd_v - jd[k]) + dP_k)
 *   landmark:       the barycentric sum of its three vertices
 * in fp32 FMAs in a fixed order for either tik_fk_set_precision setting (the
 * skinning entries as tik_fk_joints takes them: the sparse pairs, or all 55
 * weights under TIK_FK_SKIN=dense): a body's rows are the same bits for any B,
 * any place in the batch and any selection around a column. The selection
 * travels in the kernel arguments: a call uploads nothing and is
 * stream-ordered. Workspace: 1337 + 165 nb floats per body (tik_fk_joints' 1337
 * + the derivative of the 55 chain joints for every beta; 2987 at nb = 10; plus
 * one int per body on a handle with face contours); the mesh path's buffers are
 * never reserved. TIK_E_INVALID: null pointers, B <= 0, n_sel outside 1..256, a
 * joint index out of range or a contour landmark, a model without betas. */
int tik_fk_joints_shape_jacobian(tik_fk_t fk, const float* full_pose, const float* betas, const float* expression,
                                 const float* transl, int B, const int* sel_host, int n_sel,
                                 float* jac, float* joints, void* stream);
/* Bytes of device workspace the handle currently owns (constants excluded). */
long long tik_fk_workspace_bytes(tik_fk_t fk);
/* Per-launch HIP-event profile of tik_fk_forward (fk_chain, fk_blend, fk_skin,
 * fk_landmarks), tik_fk_joints (fk_chain, fk_joints) and
 * tik_fk_joints_jacobian (fk_chain, fk_jacobian; when joints are asked for,
 * tik_fk_joints' own fk_chain, fk_joints come first and the second fk_chain
 * runs only if no selected joint is made of vertices) and
 * tik_fk_joints_shape_jacobian (fk_chain, fk_shape_jacobian; with joints
 * fk_chain, fk_joints, fk_shape_jacobian, the second fk_chain as above), as
 * tik_model_profile / _count / _read. */
int tik_fk_profile(tik_fk_t fk, int max_launches);
int tik_fk_profile_count(tik_fk_t fk);
int tik_fk_profile_read(tik_fk_t fk, int i, char* label, int label_len, float* ms, double* flops, double* bytes);

/* ------------------------------------------------------------------------
 * Batched damped least squares (the Levenberg-Marquardt step of refine.py):
 * for each body b it solves
 *   (J^T W J + (mu + lambda[b]) I) delta = -(J^T W r + mu prior)
 * jac (B,m,n), r (B,m), prior (B,n) or NULL (= 0), row_w (m) non-negative row
 * weights W = diag(row_w) or NULL (= 1), lambda (B), delta (B,n); all device
 * fp32. 1 <= n <= 165, 1 <= m <= 768, mu >= 0; mu + lambda[b] > 0 is the
 * caller's promise. No handle and no workspace: one workgroup per body builds
 * the normal matrix in LDS (fp32 FMAs, rows ascending), factors it (Cholesky)
 * and runs both triangular solves in the same launch; only delta is written.
 * A pivot that is not positive writes NaN into that body's delta and nothing
 * else. A body's delta is the same bits for any B. Stream-ordered.
 * TIK_E_INVALID: null jac / r / lambda / delta, B <= 0, n or m out of range,
 * mu negative or NaN.
 * ---------------------------------------------------------------------- */
int tik_lm_solve(const float* jac, const float* r, const float* prior, const float* row_w, const float* lambda,
                 float mu, int B, int m, int n, float* delta, void* stream);

/* ------------------------------------------------------------------------
 * The same least squares with unknowns shared by the whole batch (the shape
 * step of refine.py): one system
 *   (sum_b J_b^T W J_b + (mu + lambda) I) delta = -(sum_b J_b^T W r_b + mu prior)
 * in two calls. Neither takes a handle or owns a workspace; both are
 * stream-ordered.
 * tik_lm_accumulate: jac (B,m,n), r (B,m), row_w (m) or NULL (= 1), limits as
 * tik_lm_solve (1 <= n <= 165, 1 <= m <= 768) -> partial
 * (ceil(B / TIK_LM_RUN), n (n + 1) / 2 + n) device fp32, allocated by the
 * caller. Row q holds the lower triangle of sum_b J_b^T W J_b, packed (entry
 * (i, j <= i) at i (i + 1) / 2 + j), then sum_b J_b^T W r_b, over the bodies
 * TIK_LM_RUN q .. TIK_LM_RUN q + TIK_LM_RUN - 1 that are below B. One workgroup
 * per run, everything in LDS; every entry is one fp32 FMA chain from zero,
 * bodies ascending and rows ascending within a body, so a row's bits depend on
 * its own bodies only. A sequence longer than one call accumulates each chunk
 * into its own rows of one buffer (a chunk that is a multiple of TIK_LM_RUN
 * bodies leaves the rows what one call over the whole sequence writes).
 * tik_lm_solve_sum: partial (n_part, n (n + 1) / 2 + n), prior (n) or NULL
 * (= 0), host floats mu >= 0 and lambda >= 0 -> delta (n). One workgroup adds
 * the n_part rows in ascending order, puts mu + lambda on the diagonal, forms
 * -(g + mu prior), then factors (Cholesky) and solves exactly as tik_lm_solve
 * does. mu + lambda > 0 or a full-rank sum is the caller's promise: a pivot
 * that is not positive writes NaN into delta and nothing else.
 * TIK_E_INVALID: null jac / r / partial / delta, B <= 0, n_part <= 0, n or m
 * out of range, mu or lambda negative or NaN.
 * ---------------------------------------------------------------------- */
#define TIK_LM_RUN 32   /* bodies per partial sum */
int tik_lm_accumulate(const float* jac, const float* r, const float* row_w, int B, int m, int n,
                      float* partial, void* stream);
int tik_lm_solve_sum(const float* partial, int n_part, const float* prior, float mu, float lambda, int n,
                     float* delta, void* stream);

/* ------------------------------------------------------------------------
 * The same least squares with neighbouring frames tied together (the
 * temporally smooth refinement of refine.py): F frames in S sequences,
 * sequence q the frames a = seq_starts[q] .. b - 1 = seq_starts[q + 1] - 1,
 * c_f the number of neighbours of f inside its sequence (0, 1 or 2):
 *   D_f = J_f^T W_f J_f + ((mu + lambda[q]) + smooth c_f) I
 *   b_f = -( fma(mu, prior_f, J_f^T W_f r_f) + smooth (c_f theta_f - theta_{f-1} - theta_{f+1}) )
 *   D_f delta_f - smooth delta_{f-1} - smooth delta_{f+1} = b_f
 * (neighbours inside the sequence only): the Gauss-Newton system of the cost
 * with 1/2 smooth sum_f |theta_{f+1} - theta_f|^2 added, symmetric positive
 * definite and block tridiagonal with off-diagonal blocks -smooth I.
 * jac (F,m,n), r (F,m), prior (F,n) or NULL (= 0), theta (F,n) (NULL allowed
 * only when smooth == 0), row_w NULL (= 1), (m) with row_w_stride == 0 or
 * (F,m) with row_w_stride == m, lambda (S), delta (F,n): device fp32;
 * seq_starts: device int32, S + 1 entries. 1 <= n <= TIK_LM_CHAIN_MAX_N,
 * 1 <= m <= 768, 1 <= S <= F, mu >= 0, smooth >= 0. No handle; workspace:
 * tik_lm_chain_workspace_floats(F, n) = F (n (n + 1) / 2 + n) device floats
 * owned by the caller. Stream-ordered, no host copy. Two launches:
 * 1. one workgroup per frame writes the packed lower triangle of D_f, then
 *    b_f, into workspace row f (the accumulation of tik_lm_solve);
 * 2. one workgroup per sequence, everything in LDS, block Cholesky: frames
 *    ascending S_f = D_f - smooth^2 S_{f-1}^-1 (S_a = D_a), y_f = b_f + smooth
 *    x_{f-1}, S_f = L_f L_f^T, x_f = S_f^-1 y_f, S_f^-1 = (L_f^-1)^T L_f^-1;
 *    L_f and x_f replace workspace row f; frames descending delta_{b-1} =
 *    x_{b-1}, delta_f = x_f + smooth (L_f L_f^T)^-1 delta_{f+1}.
 * Every sum is an fp32 FMA chain in a fixed order: a sequence's bits do not
 * depend on what else is in the launch, and with smooth == 0, or for a
 * sequence of one frame, delta is bit for bit tik_lm_solve's. A pivot that is
 * not positive (or NaN) at any frame writes NaN into that whole sequence's
 * delta and nothing else. A sequence whose bounds are not 0 <= a < b <= F
 * does no work; no index leaves [0, F) whatever seq_starts holds. That
 * seq_starts starts at 0, ascends strictly and ends at F is the caller's
 * promise (smplx_fk.lm_chain_starts checks it on the host).
 * TIK_E_INVALID: null jac / r / lambda / seq_starts / workspace / delta, null
 * theta with smooth > 0, F <= 0, S <= 0, S > F, n or m out of range, mu or
 * smooth negative or NaN, row_w_stride not 0 or m.
 * ---------------------------------------------------------------------- */
#define TIK_LM_CHAIN_MAX_N 96
size_t tik_lm_chain_workspace_floats(int F, int n);
int tik_lm_solve_chain(const float* jac, const float* r, const float* prior, const float* theta,
                       const float* row_w, int row_w_stride, const float* lambda, const int* seq_starts,
                       float mu, float smooth, int F, int S, int m, int n,
                       float* workspace, float* delta, void* stream);

/* ------------------------------------------------------------------------
 * The whole Levenberg-Marquardt refinement of a frame in one launch (the
 * fused path of refine.py, and the refinement inside an online stream): one
 * workgroup per frame, FK, Jacobian, normal equations, Cholesky, candidate and
 * accept rule all in LDS; only the pose (and optionally the cost row) is
 * written. Per frame, theta the 66 pose values of joints 0..21 (the other
 * joints stay at pose_mean), theta0 = prior, thetap = prev:
 *   r(theta)    = rel(FK keypoints(theta)) - rel(kps)       rel(x) = x - mean of columns 11 and 12
 *   cost(theta) = 1/2 sum_k w_k |r_k|^2 + 1/2 mu |theta - theta0|^2 + 1/2 smooth |theta - thetap|^2
 *   (J^T W J + (mu + smooth + lambda) I) delta = -(J^T W r + mu (theta - theta0) + smooth (theta - thetap))
 * the thetap terms only with prev and smooth > 0. Exactly `iters` iterations
 * from lambda = lam0: theta + delta is kept where its cost fell (lambda / 3),
 * else theta stays (3 lambda); a NaN cost or a pivot that is not positive is no
 * fall, so a frame with a NaN keypoint returns its pose unchanged with a NaN
 * cost row. poses (B,66) the start; prior (B,66) or NULL (= poses); prev (B,66)
 * or NULL; kps (B,17,3); betas: row b at betas + b betas_ld (betas_ld = 0: one
 * row for all frames) or NULL (the mean shape); joint_w: non-negative keypoint
 * weights, row b at joint_w + b joint_w_ld (0: one row of 17 shared, 17: per
 * frame) or NULL (ones); all device fp32. sel17 (host): the 17 keypoints as
 * joint indices, chain joints (< 55) or single-vertex joints (55 .. 55 + 21),
 * or NULL = COCO-17 on SMPL-X {55,57,56,59,58,16,17,18,19,20,21,1,2,4,5,7,8};
 * columns 11 and 12 are the root pair. out_poses (B,66); out_cost (B,iters+1)
 * or NULL: column 0 the start's cost, column i + 1 the kept pose's after
 * iteration i, never increasing; dbg_jac (B,51,66) and dbg_r (B,51) or NULL:
 * the first linearisation, rows root-relative (written for any iters). fp32
 * FMAs in a fixed order, no atomics: a frame's output bits do not depend on B
 * or on its place in the batch (they are not those of tik_fk_joints_jacobian /
 * tik_lm_solve: other sum orders). Both skinning table forms of the handle
 * (the pairs, TIK_FK_SKIN=dense). The selection travels in the kernel
 * arguments; no workspace, nothing uploaded, stream-ordered. iters = 0 copies
 * poses and writes cost column 0.
 * TIK_E_INVALID: null fk / poses / kps / out_poses, B <= 0, iters < 0, mu <= 0
 * or NaN, smooth < 0 or NaN, lam0 <= 0 or NaN, betas_ld not 0 or >= nb,
 * joint_w_ld not 0 or 17, a joint index out of range, a landmark of three
 * vertices or a contour landmark in sel17.
 * ---------------------------------------------------------------------- */
int tik_fk_refine(tik_fk_t fk, const float* poses, const float* prior, const float* prev, const float* kps,
                  const float* betas, int betas_ld, const float* joint_w, int joint_w_ld, const int* sel17, int iters,
                  float mu, float smooth, float lam0, int B, float* out_poses, float* out_cost, float* dbg_jac,
                  float* dbg_r, void* stream);
/* tik_fk_refine on imperfect detections; tik_fk_refine is this call with
 * (robust_sigma, flags, dbg_w) = (0, 0, NULL), the same instructions and bits.
 * robust_sigma > 0 (metres) replaces the weighted square of the data term by
 * Geman-McClure on s_k = |r_k|^2:
 *   rho(s)      = sigma^2 s / (sigma^2 + s)
 *   cost(theta) = 1/2 sum_k w_k rho(s_k) + the prior and prev terms as above
 *   omega_k     = w_k rho'(s_k) = w_k (sigma^2 / (sigma^2 + s_k))^2        (from the current pose's residual)
 *   (J^T Omega J + (mu + smooth + lambda) I) delta = -(J^T Omega r + mu (theta - theta0) + smooth (theta - thetap))
 * J^T Omega r is the exact gradient of the robust data term; the matrix is the
 * Gauss-Newton (IRLS) one: the second-derivative term of rho, which is
 * negative (it turns the full Hessian indefinite along r_k past s_k =
 * sigma^2 / 3), is dropped on purpose, so the matrix stays positive
 * definite. Accept and reject are judged on the true robust cost of the
 * candidate, and the cost row still never increases. There is no tuned sigma:
 * 0 (off) is the default everywhere.
 * flags: TIK_REFINE_SKIP_NONFINITE treats a keypoint with a NaN or Inf
 * component as missing: weight 0 and a finite target; a frame whose column 11
 * or 12 is missing has all 17 weights 0 and can move only toward prior and
 * prev. Without the flag a NaN keypoint behaves as in tik_fk_refine.
 * dbg_w (B,17) or NULL: the omega_k of the first linearisation (w_k where
 * robust_sigma = 0), written for any iters like dbg_jac / dbg_r.
 * TIK_E_INVALID before any device work: whatever tik_fk_refine refuses, a
 * robust_sigma that is negative, NaN or infinite, a bit of flags other than
 * the one defined. */
#define TIK_REFINE_SKIP_NONFINITE 1
int tik_fk_refine_robust(tik_fk_t fk, const float* poses, const float* prior, const float* prev, const float* kps,
                         const float* betas, int betas_ld, const float* joint_w, int joint_w_ld, const int* sel17,
                         int iters, float mu, float smooth, float lam0, int B, float* out_poses, float* out_cost,
                         float* dbg_jac, float* dbg_r, float robust_sigma, int flags, float* dbg_w, void* stream);

/* ------------------------------------------------------------------------
 * The keypoint loss of a pose and its gradient with respect to the pose in
 * one launch (the keypoint term of a training loss: HMR / VIBE style
 * |rel(FK(pred)) - rel(kps)|^2, back-propagated through FK): one workgroup per
 * frame, FK, residual and the analytic Jacobian in LDS (tik_fk_refine's device
 * code, one FK state, no normal equations). Per frame f, theta the 66 pose
 * values of joints 0..21 (the other joints stay at pose_mean):
 *   r          = rel(FK keypoints(theta_f, betas_f)) - rel(kps_f)    rel(x) = x - mean of columns 11 and 12
 *   loss[f]    = 1/2 sum_k w_k |r_k|^2                               (the data term of tik_fk_refine's cost)
 *   g[q]       = sum_i w_i J[i][q] r[i]     i < 51, q < 66           (J^T W r, J with root-relative rows)
 *   grad[f][q] = grad_scale g[q], or with accumulate != 0 fmaf(grad_scale, g[q], grad[f][q])
 * poses: row f at poses + f poses_ld (poses_ld >= 66; the trainer's pose
 * matrix has 68); kps (.,17,3); betas, betas_ld, joint_w, joint_w_ld, sel17
 * exactly as in tik_fk_refine; loss indexed by frame, or NULL; grad: row f at
 * grad + f grad_ld (grad_ld >= 66), or NULL; at least one of the two. All
 * device fp32 but sel17 (host). rows: device int32 with B entries, or NULL for
 * frames 0 .. B-1: workgroup b works on frame f = rows[b] for every input and
 * output, frames not listed are not touched, distinct entries are the
 * caller's promise, and NO index derived from rows is range-checked on the
 * device: an entry outside the caller's arrays reads and writes out of bounds.
 * A NaN keypoint or pose gives that frame a NaN loss and a NaN gradient row
 * and affects no other frame. fp32 FMAs in a fixed order, no atomics, one
 * writer per output element: a frame's bits do not depend on B, on its place
 * in the batch or on rows (they are not those of tik_fk_joints_jacobian).
 * Both skinning table forms of the handle. No workspace, nothing uploaded,
 * stream-ordered.
 * TIK_E_INVALID, before any device work: null fk / poses / kps, loss and grad
 * both NULL, B <= 0, poses_ld < 66, grad_ld < 66 with grad, a grad_scale that
 * is not finite, betas_ld not 0 or >= nb, joint_w_ld not 0 or 17, a joint index
 * out of range, a landmark of three vertices or a contour landmark in sel17.
 * ---------------------------------------------------------------------- */
int tik_fk_keypoint_loss(tik_fk_t fk, const float* poses, int poses_ld, const float* kps, const float* betas, int betas_ld,
                         const float* joint_w, int joint_w_ld, const int* sel17, const int* rows, int B, float* loss,
                         float* grad, int grad_ld, float grad_scale, int accumulate, void* stream);

/* ------------------------------------------------------------------------
 * The pose metrics of B frames in one launch (what a pose regressor is
 * judged by): one workgroup per frame, tik_fk_keypoint_loss's FK, then the
 * alignment in one wave's registers. Per frame f, k < 17 keypoints:
 *   x_k = rel(FK keypoints(theta_f, betas_f)), y_k = rel(kps_f), W = sum_k w_k, n = #{k : w_k > 0}
 *   out[f][0] mpjpe    = sum_k w_k |x_k - y_k| / W                      (metres; NaN when W = 0)
 *   out[f][1] pa_mpjpe = sum_k w_k |s R (x_k - mx) - (y_k - my)| / W    (NaN when n < 3)
 *   out[f][2] mpjae    = (1/22) sum_{j<22} angle(R_j^T R*_j)            (radians; NaN when target_poses == NULL)
 *   out[f][3] weight   = W
 * mx, my are the w-weighted means; R in SO(3) is the proper rotation that
 * minimises sum w |s R (x - mx) - (y - my)|^2 (Horn's quaternion form: a
 * mirrored body is not aligned by a reflection, and a planar set of keypoints
 * needs no special case), s = sum w (y - my) . R (x - mx) / sum w |x - mx|^2.
 * R_j = the rotation of theta_j + pose_mean_j, R*_j that of target_poses;
 * angle = atan2(|axial(D)|, (tr D - 1) / 2), sound at 0 and at pi.
 * poses: row f at poses + f poses_ld (poses_ld >= 66); target_poses: row f at
 * target_poses + f target_ld (target_ld >= 66), or NULL; kps (.,17,3); betas,
 * betas_ld, joint_w, joint_w_ld, sel17 and rows exactly as in
 * tik_fk_keypoint_loss (rows is NOT range-checked on the device). flags:
 * TIK_REFINE_SKIP_NONFINITE as in tik_fk_refine_robust: a keypoint with a NaN
 * or Inf component weighs 0, and a frame without column 11 or 12 has W = 0.
 * out (.,4) indexed by frame; joints_out (.,17,3) indexed by frame, or NULL:
 * the x_k. All device fp32 but sel17 (host). A pose value that is not finite
 * gives its frame NaN in all four columns; without the flag a NaN keypoint
 * gives NaN in columns 0 and 1; no other frame is affected. fp32 in a fixed
 * order (a fixed number of Jacobi sweeps, no loop until converged), no
 * atomics, one writer per output element: a frame's bits do not depend on B,
 * on its place in the batch or on rows. Both skinning table forms of the
 * handle. No workspace, nothing uploaded, stream-ordered.
 * TIK_E_INVALID, before any device work: null fk / poses / kps / out, B <= 0,
 * poses_ld < 66, target_ld < 66 with target_poses, betas_ld not 0 or >= nb,
 * joint_w_ld not 0 or 17, a bit of flags other than the one defined, a joint
 * index out of range, a landmark of three vertices or a contour landmark in
 * sel17.
 * ---------------------------------------------------------------------- */
int tik_fk_pose_metrics(tik_fk_t fk, const float* poses, int poses_ld, const float* kps, const float* betas, int betas_ld,
                        const float* joint_w, int joint_w_ld, const float* target_poses, int target_ld, const int* sel17,
                        const int* rows, int B, int flags, float* out, float* joints_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TIK_H */
