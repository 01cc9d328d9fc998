/*
 * mpinets_hip.h -- C-ABI of libmpinets_hip.so, the MI355X (gfx950) engine behind the hot path
 * of NVlabs/motion-policy-networks.
 *
 * The reference has no FFI of its own (it is pure Python); the seams this ABI
 * sits behind are the Python-level call sites cited on each entry point
 * (paths relative to /root/reference).  INTEGRATION.md shows the ctypes binding a reference
 * maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless marked "host"; plain C types only;
 *   - all tensors are dense, row-major, float32 / int32; "stride" arguments count floats;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls only enqueue (the first launch of
 *     a large-LDS kernel on a device also raises that kernel's LDS limit, once);
 *   - return 0 on success, non-zero on error (mpx_last_error() gives the text, per thread);
 *   - no call allocates or frees device memory, so every call is hipGraph-capturable
 *     (exception: none).
 */
#ifndef MPINETS_HIP_H
#define MPINETS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *mpx_stream_t;

#define MPX_NUM_FRAMES 15 /* link0..8, hand, leftfinger, rightfinger, l/r fingertip, right_gripper */

int mpx_version(void); /* 341 (unchanged: an addition, no caller of an earlier 341 library needs rebuilding): mpx_scene_generate_reference;
                          341 (unchanged, likewise): mpx_scene_generate;
                          341 (unchanged, likewise): mpx_gripper_shortcut, mpx_gripper_shortcut_cloud, struct mpx_gripper_shortcut_options;
                          341 (unchanged, likewise): mpx_franka_shortcut, mpx_franka_shortcut_cloud, struct mpx_shortcut_options; 341 (unchanged, likewise):
                          mpx_task_candidates, struct mpx_task_candidates_options; 341 (unchanged, likewise):
                          the form query mpx_linear_form; 341 (unchanged, likewise):
                          mpx_gripper_roadmap_cloud; 341 (unchanged, likewise): mpx_franka_follow_cloud,
                          mpx_franka_follow_cloud_scratch; 341 (unchanged, likewise): mpx_franka_roadmap_cloud,
                          mpx_franka_plan_cloud_seeded, MPX_FRANKA_MAX_SPHERE_RADIUS; 341 (unchanged, likewise): mpx_gripper_roadmap,
                          struct mpx_gripper_roadmap_options; 341 (unchanged, likewise): mpx_franka_follow,
                          struct mpx_follow_options; 341 (unchanged, likewise): mpx_franka_roadmap,
                          struct mpx_roadmap_options, mpx_franka_plan_seeded;
                          341: the route queries mpx_fps_route, mpx_franka_collision_route, mpx_linear_route, mpx_linear_wgrad_route,
                          mpx_pool_wgrad_route, mpx_sa_mlp_route (additions only);
                          340 (unchanged: additions, no caller of an earlier 340 library needs rebuilding): mpx_franka_cloud_collision_each,
                          mpx_franka_ik_cloud, mpx_franka_ik_cloud_scratch; 340 (unchanged, likewise): mpx_cloud_field_build,
                          mpx_cloud_field_sample, mpx_franka_plan_cloud, mpx_franka_plan_cloud_scratch, struct mpx_field_grid;
                          340 (unchanged, likewise): mpx_cloud_clean,
                          mpx_cloud_clean_scratch; 340 (unchanged, likewise): mpx_franka_cloud_collision,
                          MPX_VARIANT_CLOUD_CULL; 340 (unchanged, likewise): mpx_ball_query_set;
                          340 (unchanged, likewise): mpx_franka_ik, struct mpx_ik_options, mpx_franka_plan, struct mpx_plan_options;
                          340: mpx_pool_wgrad / mpx_pool_wgrad_scratch / mpx_pool_dgrad, mpx_linear_segmax / mpx_linear_segmax_bf16x3, mpx_pack_rows_ld / mpx_pack_rows_grad_ld (additions only);
                          330: mpx_sa3_front_bf16x3 / _pack / _pack_size / _w3_pairs (additions), the measurement hooks mpx_sa3_chain_probe / mpx_sa2_bf16x3_set_probe /
                          mpx_sa3_front_bf16x3_probe declared, mpx_sa_mlp_bf16x3_factored refuses nsample > 128;
                          320: mpx_linear_dact, mpx_segment_max_grad_act, mpx_linear_bf16x3_dact, mpx_linear_wgrad_bf16x3 (additions only); mpx_franka_collision accepts
                          frame pointers that are not 16-byte aligned;
                          310: struct mpx_policy_weights ends with sa3_pack (NULL = layer-by-layer group-all module at every
                          batch size; a caller built against the 200 header must be rebuilt), MPX_VARIANT_UNIT_QUEUE,
                          mpx_ball_query_hits rejects nsample > 256;
                          300: mpx_set_variant / mpx_get_variant, mpx_sa_mlp_bf16x3_wants_order takes nsample */
const char *mpx_last_error(void);
/* host-side query of the device the library will launch on (name buffer may be NULL) */
int mpx_device_info(char *name, int name_len, int *cu_count, int *lds_bytes);

/* ---- geometry: mpinets/geometry.py -------------------------------------------------------- */

/* TorchCuboids/TorchCylinders.__init__ + _init_frames (geometry.py:151,177-223,409-454).
 * centers [n,3], quats [n,4] (w,x,y,z; normalised here) -> inv_frames [n,4,4] row-major:
 * rows 0..2 = [R | R.(-c)], row 3 = [0 0 0 1].  R is the reference's matrix as written,
 * including `yz - wx` at both R[1][2] and R[2][1].                                          */
int mpx_prim_frames(const float *centers, const float *quats, int n, float *inv_frames,
                    mpx_stream_t stream);

/* TorchCuboids.sdf / .sdf_sequence (geometry.py:238-288, :290-347).
 * points [B,P,3] (P = N, or T*N), out [B,P] = min over unmasked cuboids; cuboids with any
 * |dim| <= 1e-8 are masked; all masked -> +inf.                                             */
int mpx_cuboid_sdf(const float *inv_frames, const float *dims, int B, int M, const float *points,
                   int P, float *out, mpx_stream_t stream);
/* TorchCylinders.sdf / .sdf_sequence (geometry.py:456-507, :509-568). radii/heights [B,M]. */
int mpx_cylinder_sdf(const float *inv_frames, const float *radii, const float *heights, int B,
                     int M, const float *points, int P, float *out, mpx_stream_t stream);
/* TorchSpheres.sdf / .sdf_sequence (geometry.py:87-123). centers [B,M,3], radii [B,M].     */
int mpx_sphere_sdf(const float *centers, const float *radii, int B, int M, const float *points,
                   int P, float *out, mpx_stream_t stream);

/* ---- robot geometry: robofin FrankaSampler / FrankaCollisionSampler call sites ------------ */

/* FK of the Franka Panda chain: q [B,7] -> frames [B,15,12] (R row-major 3x3, then t).
 * Replaces FrankaSampler.end_effector_pose / FrankaRobot.fk (model.py:275,
 * run_inference.py:176-178).  `finger` = prismatic finger opening (0.025 in the reference). */
int mpx_franka_fk(const float *q, int B, float finger, float *frames, mpx_stream_t stream);

/* FrankaSampler.sample (model.py:250, run_inference.py:64,111,169, data_loader.py:180-185):
 * out[b, j, 0:3] = frame[b, link[src]] * table[src], src = subset ? subset[j] : j.
 * out is addressed as out + b*out_batch_stride + j*out_point_stride (floats), which lets the
 * call write straight into the xyz slab `xyz[:, :n_out, :3]` (model.py:180-181).            */
int mpx_franka_cloud(const float *q, int B, float finger, const float *table_pts,
                     const int32_t *table_link, const int32_t *subset, int n_out, float *out,
                     int64_t out_batch_stride, int out_point_stride, mpx_stream_t stream);

/* FrankaSampler.sample_end_effector (run_inference.py:66-69, data_loader.py:158-161):
 * poses [B,4,4] row-major; out[b,j] = pose[b] * table[src].                                 */
int mpx_pose_cloud(const float *poses, int B, const float *table_pts, const int32_t *subset,
                   int n_out, float *out, int64_t out_batch_stride, int out_point_stride,
                   mpx_stream_t stream);

/* FrankaCollisionSampler.compute_spheres (model.py:300): centres [B,S,3] of the S table
 * spheres (sph_centers [S,3] link-local, sph_link [S]) at configuration q [B,7].           */
int mpx_franka_spheres(const float *q, int B, float finger, const float *sph_centers,
                       const int32_t *sph_link, int S, float *out, mpx_stream_t stream);

/* Fused swept-sphere collision check, model.py:293-314, for q [B,T,7]:
 *   flags[b] |= any_{t,s} min(cuboid_sdf, cylinder_sdf)(centre[b,t,s]) <= sph_radii[s]
 * flags int32 [B] is OR-ed into (caller zeroes it); min_sdf [B,T,S] optional (may be NULL).
 * Either primitive set may be empty (M = 0).  The frame arrays are read fastest when they are
 * 16-byte aligned (the classes' inv_frames always are); unaligned pointers are accepted and
 * take a slower kernel with the same results.                                                */
int mpx_franka_collision(const float *q, int B, int T, float finger, const float *sph_centers,
                         const float *sph_radii, const int32_t *sph_link, int S,
                         const float *cub_frames, const float *cub_dims, int M1,
                         const float *cyl_frames, const float *cyl_radii,
                         const float *cyl_heights, int M2, int32_t *flags, float *min_sdf,
                         mpx_stream_t stream);

/* Swept-sphere check of q [B,T,7] against one POINT CLOUD per environment -- the scene as the policy sees it (a depth
 * cloud, a captured cloud, the scene rows of the xyz slab), no primitives needed.  Point i of environment b is the three
 * floats at cloud + b*cloud_batch_stride + i*cloud_point_stride (strides in floats, point stride >= 3: `xyz[:, 2048:6144,
 * :3]` of a [B,6272,4] slab is read in place); counts (optional int32 [B]) = how many of the N rows of environment b
 * exist, clamped to [0, N] on the device (NULL: all N).
 *   c      = centre of sphere s at waypoint (b,t): the arithmetic of mpx_franka_spheres, bit for bit
 *   d2     = fma(dz,dz, fma(dx,dx, dy*dy)) with dx = c.x - p.x, dy, dz likewise, in float32 (the library's one squared
 *            distance; MPX_SQDIST_XFIRST builds do not change this file)
 *   R      = (sph_radii[s] + point_radius) + clearance in float32 (the caller keeps it >= 0: the test squares it)
 *   hit    : d2 <= R*R;  flags[b] |= 1 if any (waypoint, sphere, existing point) of environment b hits.  flags int32 [B]
 *            is OR-ed into (caller zeroes it, as for mpx_franka_collision)
 *   best   = +inf, then `if (d2 < best) best = d2, nearest = i` over i ascending: the LOWEST index wins a tie; a point
 *            with a NaN or infinite coordinate never hits and is never nearest; an environment without points gives no
 *            hit, min_dist = +inf, nearest = -1
 *   min_dist [B,T,S] (optional) = sqrtf(best) - point_radius;  nearest int32 [B,T,S] (optional) = the index behind best
 * This is sphere-CENTRE to POINT distance: a surface sampled at spacing h can pass between the points of its cloud, and
 * point_radius is the caller's way to close that gap (about h / 2 for a gap-free cover of a flat patch).
 * With min_dist and nearest both NULL ("flags only") a workgroup may skip points outside the box of its spheres and
 * stop at the first hit (MPX_VARIANT_CLOUD_CULL); the flags are the same bit for bit.  S <= 64, point_radius >= 0.
 * A workgroup takes MPX_CLOUD_TC waypoints of one environment and walks the cloud in tiles of MPX_CLOUD_TILE points. */
#define MPX_CLOUD_TC 64
#define MPX_CLOUD_TILE 256
int mpx_franka_cloud_collision(const float *q, int B, int T, float finger, const float *sph_centers,
                               const float *sph_radii, const int32_t *sph_link, int S, const float *cloud,
                               int64_t cloud_batch_stride, int cloud_point_stride, int N, const int32_t *counts,
                               float point_radius, float clearance, int32_t *flags, float *min_dist,
                               int32_t *nearest, mpx_stream_t stream);

/* The same check with ONE VERDICT PER WAYPOINT: hit int32 [B,T] is WRITTEN (not OR-ed), every entry exactly once, 1 or 0.
 * hit[b,t] = 1 exactly when mpx_franka_cloud_collision, called on the single configuration q[b,t] (B = 1, T = 1) against
 * environment b's cloud with the same strides, counts[b], point_radius and clearance, would set its flag: the same
 * centres, the same d2, the same R = (sph_radii[s] + point_radius) + clearance and d2 <= R*R, non-finite points never hit.
 *   active int32 [B,T] (optional; NULL: every waypoint is tested): a waypoint with active[b,t] == 0 is not tested -- its q
 *   is not even read -- and gets hit = 0.
 *   N == 0, counts[b] <= 0 or S == 0 writes zeros; B == 0 or T == 0 launches nothing.  Refused: what
 *   mpx_franka_cloud_collision refuses, and hit == NULL.  No allocation, no global atomics.
 * The same kernel template: a workgroup takes MPX_CLOUD_TC waypoints of one environment; with MPX_VARIANT_CLOUD_CULL the
 * box is that of the ACTIVE waypoints' spheres and the workgroup stops after a tile once every active waypoint of its
 * chunk has a hit (not at the first hit).  The verdicts depend on the inputs alone: not on the launch shape, the variant
 * or the order in which points are staged.                                                                            */
int mpx_franka_cloud_collision_each(const float *q, int B, int T, float finger, const float *sph_centers,
                                    const float *sph_radii, const int32_t *sph_link, int S, const float *cloud,
                                    int64_t cloud_batch_stride, int cloud_point_stride, int N, const int32_t *counts,
                                    float point_radius, float clearance, const int32_t *active, int32_t *hit,
                                    mpx_stream_t stream);

/* rollout joint update, model.py:171-173 + utils.py:207-209:
 *   q_norm_out = clamp(q_norm + dq, -1, 1);  q_out = (q_norm_out + 1) * (hi - lo) / 2 + lo
 * limits [7,2] device; either output may alias q_norm; environments with frozen[b] != 0
 * (optional int32 [B]) keep their configuration.                                            */
int mpx_joint_step(const float *q_norm, const float *dq, const float *limits, int B,
                   float *q_norm_out, float *q_out, const int32_t *frozen, mpx_stream_t stream);

/* early-stop test of rollout_until_success (run_inference.py:176-187), on the device:
 *   success = |t(right_gripper(q)) - t(target)| < pos_tol  &&  cos(angle(R R_t^T)) > cos_rot_tol
 * target_poses [B,4,4] row-major.  done int32 [B] is OR-ed (a set flag freezes that environment in
 * mpx_joint_step); steps (optional) counts the policy steps taken until done; pos_err / cos_angle
 * (optional) [B] return the two measured quantities.                                            */
int mpx_franka_success(const float *q, const float *target_poses, int B, float finger, float pos_tol,
                       float cos_rot_tol, int32_t *done, int32_t *steps, float *pos_err,
                       float *cos_angle, mpx_stream_t stream);

/* Batched trajectory metrics (row N3; mpinets/metrics.py:311-384, 410-434 without PyBullet):
 * traj [B,T,7] joint angles, lengths (optional int32 [B]) valid waypoints per trajectory,
 * target_poses [B,4,4] (right_gripper), limits [7,2].  Per trajectory: final position error [cm],
 * final orientation error [deg], end-effector path lengths (m, deg), joint-limit violation flag,
 * self-collision flag.  Self collision uses the in-repo Geometric-Fabrics model
 * (config/franka_fabric_config.yaml:120-140: base body cylinder vs spheres on link7 / hand /
 * finger tips) -- NOT PyBullet's mesh test like the reference Evaluator.                        */
int mpx_trajectory_metrics(const float *traj, const int32_t *lengths, const float *target_poses,
                           const float *limits, int B, int T, float finger, float *pos_err_cm,
                           float *orient_err_deg, float *path_pos, float *path_orient_deg,
                           int32_t *limit_violation, int32_t *self_collision, mpx_stream_t stream);

/* Batched collision-free inverse kinematics (robofin FrankaRobot.ik / FrankaRealRobot.collision_free_ik, called by the
 * reference's problem generators: data_pipeline/environments/tabletop_environment.py:395, cubby_environment.py:546,
 * dresser_environment.py:496).  Damped least squares with restarts: one wave per problem, MPX_IK_SEEDS = 64 starts, one
 * per lane.  Start 0 is row b of q_init (NULL: the neutral pose), clamped into the limits; starts 1..63 are uniform in
 * the limits, drawn from Philox keyed by (seed, GLOBAL problem id = env_offset + b, start), so a shard of a larger
 * batch computes what one process computes.  Every start runs `iterations` steps
 *   dq = J^T (J J^T + lambda^2 I)^-1 [p_t - p ; rotvec(R_t R^T)],  dq scaled to max |dq_j| <= step_clip,  q clamped to limits
 * and CONVERGED means: the right_gripper frame that mpx_franka_fk computes for the final q is within pos_tol [m] and
 * rot_tol [rad] of the target (angle = atan2(|vee(E - E^T)| / 2, (trace E - 1) / 2), E = R_t R^T; tested in float32 as
 * error <= tol * MPX_IK_ACCEPT_SHARE (- MPX_IK_ACCEPT_ANGLE_MARGIN for the angle), so that a caller who re-checks the
 * frame in other arithmetic finds it inside the tolerances as stated).  Converged starts are then tested in start order against the problem's primitives
 * (min(cuboid_sdf, cylinder_sdf)(sphere centre) <= sph_radii[s] + clearance is a hit: with clearance 0 the test of
 * mpx_franka_collision) and, with check_self, against the self-collision model of mpx_trajectory_metrics; the result is
 * the LOWEST start that converged and has no hit.
 *   target_poses [B,4,4] row-major (right_gripper), limits [7,2], sphere table as for mpx_franka_collision (S <= 64,
 *   S = 0 with M1 = M2 = 0: no environment test), cub_* [B,M1,..] / cyl_* [B,M2,..] as for mpx_franka_collision
 *   (M1, M2 <= 64; zero-volume rows are skipped).
 *   q_out [B,7]; status int32 [B]: 0 solved, 1 some start converged but every converged start has a hit, 2 no start
 *   converged; rows with status != 0 are NaN.
 *   all_q [B,64,7] (optional): every start's final q, converged or not.  all_status int32 [B,64] (optional): bit 0
 *   converged, bit 1 environment hit, bit 2 self hit; when it is passed EVERY converged start is tested (otherwise the
 *   sweep stops at the first free one); q_out and status do not depend on it.                                        */
#define MPX_IK_SEEDS 64
#define MPX_IK_DEFAULT_ITERATIONS 64
#define MPX_IK_DEFAULT_LAMBDA 0.05f
#define MPX_IK_DEFAULT_STEP_CLIP 0.5f
#define MPX_IK_DEFAULT_POS_TOL 1e-3f          /* 1 mm */
#define MPX_IK_DEFAULT_ROT_TOL 8.7266463e-3f  /* 0.5 degrees */
#define MPX_IK_ACCEPT_SHARE 0.9999f
#define MPX_IK_ACCEPT_ANGLE_MARGIN 2e-6f
typedef struct mpx_ik_options { /* NULL options: the defaults above, clearance 0, check_self 0 */
  int iterations;               /* >= 1, the same for every start (no early exit)  */
  float lambda, step_clip;      /* damping (> 0) and the largest joint step [rad]  */
  float pos_tol, rot_tol;       /* acceptance: metres, radians                    */
  float clearance;              /* added to every sphere radius in the environment test */
  int check_self;               /* non-zero: also reject self collisions          */
} mpx_ik_options;
int mpx_franka_ik(const float *target_poses, int B, float finger, const float *limits, const float *q_init,
                  const float *sph_centers, const float *sph_radii, const int32_t *sph_link, int S,
                  const float *cub_inv_frames, const float *cub_dims, int M1, const float *cyl_inv_frames,
                  const float *cyl_radii, const float *cyl_heights, int M2, const mpx_ik_options *options,
                  uint64_t seed, int64_t env_offset, float *q_out, int32_t *status, float *all_q,
                  int32_t *all_status, mpx_stream_t stream);

/* mpx_franka_ik against one POINT CLOUD per environment: the lowest start that converges and is free of the cloud (and,
 * with check_self, of the robot itself).  The starts, the iterations, the acceptance test and the self bit are
 * mpx_franka_ik's -- its kernel runs, without primitives -- so for the same targets, limits, q_init, options, seed and
 * env_offset every start's final q and its bits 0 and 2 are bit-equal to what mpx_franka_ik returns in all_q / all_status.
 *   Bit 1 of a converged start is mpx_franka_cloud_collision_each's verdict on that start's q against environment b's
 *   cloud (addressed, trimmed by counts and inflated by point_radius exactly as there), with clearance =
 *   options->clearance; it is 0 on every start that did not converge (those are not tested: `active` = converged).  The
 *   result is the LOWEST start whose bits equal 1.
 *   q_out, status, NaN rows, all_q and all_status: as for mpx_franka_ik.  Every converged start is tested whether or not
 *   all_status is passed (the cloud kernel's own stop -- every active start of a chunk has hit -- is the only one), so
 *   q_out and status cannot depend on it.
 *   cloud == NULL or N == 0: no environment test (S may then be 0).  Refused: N > 0 with S == 0, point_radius < 0, a point
 *   stride below 3, a scratch that is NULL (B > 0), smaller than mpx_franka_ik_cloud_scratch(B) or not 16-byte aligned,
 *   and what mpx_franka_ik and mpx_franka_cloud_collision_each refuse.  No allocation; everything is enqueued on `stream`;
 *   B == 0 launches nothing.
 *   scratch: mpx_franka_ik_cloud_scratch(B) = B * 64 * (7 + 3) * 4 bytes (every start's q, bits, active flag, verdict);
 *   -1 for B < 0.                                                                                                    */
int64_t mpx_franka_ik_cloud_scratch(int B);
int mpx_franka_ik_cloud(const float *target_poses, int B, float finger, const float *limits, const float *q_init,
                        const float *sph_centers, const float *sph_radii, const int32_t *sph_link, int S,
                        const float *cloud, int64_t cloud_batch_stride, int cloud_point_stride, int N, const int32_t *counts,
                        float point_radius, const mpx_ik_options *options, uint64_t seed, int64_t env_offset,
                        float *q_out, int32_t *status, float *all_q, int32_t *all_status,
                        void *scratch, int64_t scratch_bytes, mpx_stream_t stream);

/* Batched collision-free trajectory planning between two configurations (what the reference's data generator asks of OMPL
 * AIT* + Geometric Fabrics and then filters with verify_trajectory, data_pipeline/gen_data.py:106-153, 396-430).  This is a
 * LOCAL optimiser, not AIT*: covariant gradient descent (CHOMP form) on a T-waypoint joint-space trajectory with fixed
 * endpoints, K = options->candidates candidates per problem; one workgroup per problem, one wave per candidate, one lane
 * per waypoint.  A returned trajectory is valid by THIS library's sphere model (mpx_franka_collision's spheres against
 * the primitives, mpx_trajectory_metrics' self test), not by PyBullet's meshes.
 *   Candidates.  L_t = q_start + s_t (q_goal - q_start), s_t = t / (T-1).  Candidate 0 is L; candidate k >= 1 is
 *   L_t + sin(pi s_t) delta_k, delta_k[j] = spread (2u - 1) (hi_j - lo_j) / 2, clamped into the limits.  u = u01 of word
 *   j (j < 4) of Philox4x32-10(counter = {2k, GLOBAL problem id = env_offset + b, stream 14, 0}, key = seed) or word j - 4
 *   of the block with counter word 0 = 2k + 1: a shard of a larger batch computes what one process computes.  Waypoints 0
 *   and T-1 are never touched: they come back bit-equal to q_start / q_goal.
 *   One iteration, for every interior waypoint t = 1..n (n = T-2), all from the trajectory of the previous iteration:
 *     x_s = the sphere centre mpx_franka_spheres computes; d_s = min over live primitives of sdf(x_s) - r_s - clearance;
 *     c'(d) = -1 (d < 0), (d - epsilon) / epsilon (0 <= d < epsilon), 0 otherwise; n_s = gradient at x_s of the arg-min
 *     primitive's SDF (ties: lowest index, cuboids before cylinders; the derivative of the function mpx_cuboid_sdf /
 *     mpx_cylinder_sdf evaluate, pulled to the world by the transpose of the stored inverse frame's 3x3);
 *     g_t[j] = sum_s c'(d_s) n_s . (z_j x (x_s - o_j)) over the revolute joints j upstream of the sphere's link;
 *     q_t <- clamp(q_t - step (smooth_weight (q_t - L_t) + sum_u M[t,u] g_u), lo, hi),
 *     M[t,u] = min(t,u) (n + 1 - max(t,u)) / (n + 1): the inverse of the fixed-endpoint velocity-smoothness metric A
 *     (tridiagonal 2, -1), for which A^-1 grad(smoothness) = q - L.
 *   Every candidate runs `iterations` steps (0: the candidates as drawn), no early exit.
 *   Validity.  Every segment is split into `substeps` pieces: refined configuration r = t substeps + i is
 *   fma((float)i / (float)substeps, q_{t+1} - q_t, q_t) in float32 (i = 0: q_t itself), r = 0 .. (T-1) substeps.  A
 *   candidate is INVALID if a refined configuration has a sphere with sdf <= r_s + clearance + check_margin (bit 0 of
 *   all_status), or, with check_self, a self-test sphere closer than 0.15 + radius + check_margin to the base segment
 *   (mpx_trajectory_metrics' model; bit 1), or if a third difference ((q3-q2)-(q2-q1)) - ((q2-q1)-(q1-q0)) of its T
 *   waypoints exceeds max_jerk * 0.9999 in absolute value (gen_data.py:82, 327-344; bit 2).  check_margin makes a caller
 *   who interpolates and judges in other arithmetic agree (an ulp of q moves a sphere by ~1e-7 m).
 *   The result is the LOWEST valid candidate.  status int32 [B]: 0 solved; 1 no valid candidate; 2 an endpoint is not
 *   finite, outside the limits or itself invalid by the tests above (no planning is done).  traj rows with status != 0
 *   are NaN; choice (optional int32 [B]) is the candidate taken or -1; all_traj [B,K,T,7] / all_status int32 [B,K]
 *   (optional) hold every candidate's final trajectory and bits (status 2: all_traj NaN, all_status 7).
 *   q_start, q_goal [B,7]; limits [7,2]; sphere table and primitives exactly as for mpx_franka_ik (S <= 64,
 *   M1, M2 <= 64, zero-volume rows skipped, S = 0 with M1 = M2 = 0: no environment term); 2 <= T <= MPX_PLAN_MAX_T.    */
#define MPX_PLAN_MAX_T 64
#define MPX_PLAN_MAX_CANDIDATES 16
#define MPX_PLAN_DEFAULT_CANDIDATES 8
#define MPX_PLAN_DEFAULT_ITERATIONS 20
#define MPX_PLAN_DEFAULT_STEP 2e-4f
#define MPX_PLAN_DEFAULT_SMOOTH_WEIGHT 20.0f
#define MPX_PLAN_DEFAULT_EPSILON 0.05f
#define MPX_PLAN_DEFAULT_SPREAD 0.5f
#define MPX_PLAN_DEFAULT_SUBSTEPS 4
#define MPX_PLAN_DEFAULT_CHECK_MARGIN 1e-4f
#define MPX_PLAN_DEFAULT_MAX_JERK 0.15f
#define MPX_PLAN_JERK_SHARE 0.9999f
typedef struct mpx_plan_options { /* NULL options: the defaults above, clearance 0, check_self 1 */
  int candidates;                 /* 1 .. MPX_PLAN_MAX_CANDIDATES                                  */
  int iterations;                 /* >= 0, the same for every candidate (no early exit)            */
  float step, smooth_weight;      /* step > 0; smooth_weight >= 0 pulls toward the straight line   */
  float epsilon;                  /* > 0: width [m] of the band in which an obstacle repels         */
  float spread;                   /* candidates >= 1: amplitude, as a share of the half joint range */
  int substeps;                   /* >= 1: pieces per segment in the validity sweep                */
  float check_margin;             /* >= 0 [m], added to the radii in the validity sweep only       */
  float clearance;                /* [m], added to the radii in the cost AND the validity sweep    */
  float max_jerk;                 /* largest third difference [rad]                                */
  int check_self;                 /* non-zero: self collisions invalidate a candidate              */
} mpx_plan_options;
int mpx_franka_plan(const float *q_start, const float *q_goal, int B, int T, float finger, const float *limits,
                    const float *sph_centers, const float *sph_radii, const int32_t *sph_link, int S,
                    const float *cub_inv_frames, const float *cub_dims, int M1, const float *cyl_inv_frames,
                    const float *cyl_radii, const float *cyl_heights, int M2, const mpx_plan_options *options,
                    uint64_t seed, int64_t env_offset, float *traj, int32_t *status, int32_t *choice, float *all_traj,
                    int32_t *all_status, mpx_stream_t stream);

/* mpx_franka_plan with caller-supplied candidates: seeds [B,Ks,T,7], Ks >= 0, candidates + Ks <= MPX_PLAN_MAX_CANDIDATES.
 *   Candidates 0 .. K-1 (K = options->candidates) are drawn and optimised exactly as by mpx_franka_plan; candidate K + i
 *   starts from seeds[b,i]: its interior waypoints clamped into the limits, waypoints 0 and T-1 replaced by q_start / q_goal.
 *   L stays the straight line for every candidate (the smoothness term's q - L pulls a seed toward the line as it pulls a
 *   drawn candidate).  A seed with an entry that is not finite is not optimised: its all_traj rows are NaN and its
 *   all_status is 7.  Iterations, validity, the bits, "the LOWEST valid candidate" and status 2 are mpx_franka_plan's;
 *   all_traj is [B,K+Ks,T,7], all_status [B,K+Ks], choice counts over K + Ks.  Hence: with Ks = 0 every output is bit-equal
 *   to mpx_franka_plan's (it is that launch); with any Ks candidates 0 .. K-1 are bit-equal, and a row mpx_franka_plan
 *   solves comes back identical.  seeds may be NULL when Ks = 0.                                                          */
int mpx_franka_plan_seeded(const float *q_start, const float *q_goal, int B, int T, float finger, const float *limits,
                           const float *sph_centers, const float *sph_radii, const int32_t *sph_link, int S,
                           const float *cub_inv_frames, const float *cub_dims, int M1, const float *cyl_inv_frames,
                           const float *cyl_radii, const float *cyl_heights, int M2, const mpx_plan_options *options,
                           uint64_t seed, int64_t env_offset, const float *seeds, int Ks, float *traj, int32_t *status,
                           int32_t *choice, float *all_traj, int32_t *all_status, mpx_stream_t stream);

/* A lazy probabilistic roadmap per problem: the GLOBAL half of what the reference asks of OMPL, whose path seeds the local
 * optimiser above (mpx_franka_plan_seeded smooths and judges it as it judges its own candidates).  One workgroup per
 * problem; the result depends on the inputs alone (no atomics on results, no dependence on lane timing).
 *   Nodes.  V = options->nodes, 2 <= V <= MPX_ROADMAP_MAX_NODES.  Node 0 is q_start, node 1 q_goal; node v >= 2 has
 *   q_j = fma(u_j, hi_j - lo_j, lo_j), u_j = u01 of word j (j < 4) of Philox4x32-10(counter = {2v, GLOBAL problem id =
 *   env_offset + b, stream 16, 0}, key = seed) or word j - 4 of the block with counter word 0 = 2v + 1: a shard of a
 *   larger batch computes what one process computes.
 *   A configuration is VALID by mpx_franka_plan's validity test, unchanged: no sphere with sdf <= r_s + clearance +
 *   check_margin, and with check_self no self-test sphere inside 0.15 + radius + check_margin.
 *   status int32 [B]: 2 an endpoint is not finite, outside the limits or invalid (mpx_franka_plan's rule; no search is
 *   done, rounds = 0); 0 a path was found; 1 none was.  Invalid nodes other than the endpoints take no part in the search.
 *   Edge (a,b), a < b: d = q_b - q_a, w = sqrtf(fma(d_6, d_6, ... fma(d_1, d_1, d_0 d_0))) (the same bits for (b,a));
 *   n = min(2^20, max(1, (int)ceilf(w / resolution))) pieces; interior configuration i = 1 .. n-1 is
 *   fma((float)i / (float)n, d, q_a).  The edge is BLOCKED exactly when an interior configuration is invalid; an edge with
 *   w > connect_radius does not exist.
 *   Search, at most max_rounds rounds.  A round finds the shortest path from node 0 to node 1 over the valid nodes and the
 *   edges that are not blocked (untested edges count as free) by Jacobi sweeps to a fixed point: d_0 = 0, every other
 *   d = +inf, no predecessors; a sweep reads the previous sweep's distances only and gives every valid node v != 0
 *   d_v <- min(d_v, min_u (d_u + w_uv)) in float32, evaluated for u = 0 .. V-1 ascending with a strict "<" against the
 *   running minimum that starts at the old d_v; the predecessor becomes the u that last lowered it (the lowest u among
 *   equal sums) and is kept when none did.  The sweeps end when one changes no distance.  d_1 = +inf: status 1.  Else every
 *   untested edge of the path 1, pred(1), .. 0 is tested in full and becomes free or blocked; if none is blocked the path is
 *   the answer (status 0), else the next round searches again.  Rounds used up: status 1.
 *   path int32 [B,V]: the node indices from 0 to 1, then -1; hops int32 [B]: its edges.  Rows with status != 0: hops 0,
 *   path all -1.  Optional: nodes [B,V,7]; edge_state uint8 [B,V,V], symmetric, 0 untested / 1 free / 2 blocked, the
 *   diagonal 1 for a valid node and 2 for an invalid one; rounds int32 [B], the searches run.
 *   traj [B,T,7], 2 <= T <= MPX_PLAN_MAX_T, the seed trajectory.  A one-edge path gives mpx_franka_plan's line L_t bit for
 *   bit (not resampled, not smoothed).  Otherwise, with c_0 = 0, c_{i+1} = c_i + w_i summed in path order in float32 and
 *   s_t = ((float)t / (float)(T-1)) c_hops: waypoint t lies on the last edge i with c_i <= s_t, at
 *   fma(f, p_{i+1} - p_i, p_i), f = min((s_t - c_i) / w_i, 1) (0 if w_i = 0), p_i the path's nodes in path order; then
 *   smooth_passes passes of q_t <- fma(0.25, q_{t-1} + q_{t+1}, 0.5 q_t) on t = 1 .. T-2, each from the previous pass (the
 *   corners are rounded so that the optimiser's third-difference test has a chance).  Waypoints 0 and T-1 are bit-equal to
 *   q_start / q_goal.  Rows with status != 0 are NaN.
 *   q_start, q_goal, limits, the sphere table and the primitives exactly as for mpx_franka_plan.  No allocation, no
 *   scratch, no global atomics; everything is enqueued on `stream` (capturable).  B == 0 launches nothing.              */
#define MPX_ROADMAP_MAX_NODES 256
#define MPX_ROADMAP_DEFAULT_NODES 64
#define MPX_ROADMAP_DEFAULT_RESOLUTION 0.05f
#define MPX_ROADMAP_DEFAULT_MAX_ROUNDS 64
#define MPX_ROADMAP_DEFAULT_SMOOTH_PASSES 8
typedef struct mpx_roadmap_options { /* NULL options: the defaults above, connect_radius +inf, check_margin
                                        MPX_PLAN_DEFAULT_CHECK_MARGIN, clearance 0, check_self 1 */
  int nodes;                         /* 2 .. MPX_ROADMAP_MAX_NODES, start and goal included              */
  float resolution;                  /* > 0 [rad]: the longest piece of an edge (joint-space 2-norm)     */
  float connect_radius;              /* [rad], longer edges do not exist; +inf: the complete graph       */
  int max_rounds;                    /* >= 1: searches before giving up                                   */
  int smooth_passes;                 /* >= 0: (1/4, 1/2, 1/4) passes over the resampled polyline          */
  float check_margin;                /* >= 0 [m], as in mpx_plan_options                                  */
  float clearance;                   /* [m], added to the radii                                           */
  int check_self;                    /* non-zero: self collisions invalidate a configuration              */
} mpx_roadmap_options;
int mpx_franka_roadmap(const float *q_start, const float *q_goal, int B, int T, float finger, const float *limits,
                       const float *sph_centers, const float *sph_radii, const int32_t *sph_link, int S,
                       const float *cub_inv_frames, const float *cub_dims, int M1, const float *cyl_inv_frames,
                       const float *cyl_radii, const float *cyl_heights, int M2, const mpx_roadmap_options *options,
                       uint64_t seed, int64_t env_offset, float *traj, int32_t *status, int32_t *path, int32_t *hops,
                       float *nodes, uint8_t *edge_state, int32_t *rounds, mpx_stream_t stream);

/* A reactive follower of an end-effector path, its retiming and its verdict: where the reference's data generator runs
 * Geometric Fabrics along the global plan, downsamples to 50 waypoints and filters with verify_trajectory
 * (data_pipeline/gen_data.py:156-307, 433-528: the 'hybrid_solutions' key).  This is a STAND-IN, NOT Lula's fabric and claims
 * no parity with it: a damped second-order joint-space system driven by mpx_franka_ik's damped-least-squares direction
 * toward the current guide pose, mpx_franka_plan's obstacle gradient, a joint-limit barrier and viscous damping, under
 * a joint speed limit.  One wave per problem, lane = collision sphere in the obstacle term; no randomness (no seed, no
 * env_offset): row b depends on row b's inputs alone, and the obstacle sum is reduced across lanes in a fixed order.
 *   q_start [B,7]; poses [B,W,4,4] row-major right_gripper guide poses, 1 <= W <= MPX_FOLLOW_MAX_POSES; limits [7,2], the
 *   sphere table and the primitives exactly as for mpx_franka_ik (S <= 64, M1, M2 <= 64, zero-volume rows skipped);
 *   2 <= T <= MPX_PLAN_MAX_T; v_init [B,7] (NULL: zeros); progress_init int32 [B,3] = {waypoint w, steps spent on it n_w,
 *   finished flag} (NULL: {0, 0, 0}).
 *   One step from (q, v, w, n_w), p_w / R_w the position / rotation of guide pose w:
 *     1. FK of q: p, R the right_gripper frame; dist = |p_w - p|.
 *     2. Switch: if w < W-1 and (dist <= switch_radius or n_w >= switch_steps): w <- w+1, n_w <- 0, dist recomputed for the
 *        new w.  At most one advance per step.
 *     3. Stop: if w was W-1 ON ENTRY to the step and (dist < final_radius or n_w >= final_steps): the row is FINISHED and
 *        takes no step, now or later.
 *     4. Attractor: e = [p_w - p ; rotvec(R_w R^T)], u = J^T (J J^T + lambda^2 I)^-1 e scaled so that max |u_j| <= step_clip:
 *        mpx_franka_ik's dq, statement for statement.
 *     5. Obstacle: g = mpx_franka_plan's g_t for this one configuration (the same c'(d), epsilon, clearance, arg-min tie
 *        rule and upstream-joint mask); 0 without live primitives or with S = 0.
 *     6. a_j = attract u_j - repel g_j + limit_gain (max(0, (lo_j + limit_band) - q_j) - max(0, q_j - (hi_j - limit_band)))
 *              - damping v_j.
 *     7. q'_j = q_j + dt v_j (position first, as gen_data.py:283-284); v'_j = clamp(v_j + dt a_j, -speed_limit, speed_limit);
 *        q'_j is clamped into the limits, and where the clamp moved it v'_j = 0.  n_w <- n_w + 1.
 *   At most options->max_steps steps are taken (no unbounded loop on the device: max_steps <= MPX_FOLLOW_MAX_STEPS is
 *   checked on the host, the retiming search is a bisection of fixed length).
 *   Dense path.  path[0] = q_start, path[i] = q after step i; arc[0] = 0, arc[i] = arc[i-1] + |path[i] - path[i-1]|_2
 *   (sqrtf of the fma chain over j = 0..6, in float32); n = steps[b] <= max_steps.  path [B,max_steps+1,7] and arc
 *   [B,max_steps+1] are caller-provided device buffers (required), written for 0..n only.
 *   Retiming to T waypoints of constant arc-length spacing (gen_data.py's downsample): s_t = ((float)t / (float)(T-1)) arc[n];
 *   i = the largest index with arc[i] <= s_t, capped at n-1; f = clamp((s_t - arc[i]) / (arc[i+1] - arc[i]), 0, 1), 0 for a
 *   zero denominator; q_t = fma(f, path[i+1] - path[i], path[i]).  Waypoints 0 and T-1 are path[0] and path[n] bit for
 *   bit; with n = 0 all T waypoints are q_start.
 *   Verdict on the T waypoints, bits int32 [B]: bits 0-2 are mpx_franka_plan's validity tests unchanged (the refined sweep
 *   with substeps, check_margin, clearance and check_self; third differences against max_jerk * MPX_PLAN_JERK_SHARE);
 *   bit 3 (MPX_FOLLOW_BIT_MISS) is !(|p_{W-1} - p(q_{T-1})| <= miss_tol * MPX_FOLLOW_MISS_SHARE) (gen_data.py:420).  There
 *   is no joint-limit bit: every waypoint is a convex combination of configurations clamped into the limits.
 *   status int32 [B]: 0 valid (bits == 0); 1 followed but bits != 0; 2 bad input -- q_start not finite or outside the
 *   limits, a guide pose with an entry of its first three rows not finite, with progress_init == NULL (a fresh rollout)
 *   q_start itself failing mpx_franka_plan's configuration test, or (stated here, no other entry has them) v_init not
 *   finite, progress_init with w outside 0 .. W-1 or n_w < 0 -- which takes no steps: steps 0, bits 15.  A CONTINUED
 *   rollout (progress_init given) is not refused for a state in collision: the dense path may graze an obstacle, a
 *   controller must be able to step on from any state it produced, and the verdict judges the trajectory.
 *   steps int32 [B]; traj [B,T,7], NaN where status != 0; traj_any [B,T,7] (optional) holds the status-1 rows too (NaN
 *   on status 2).  Optional q_end, v_end [B,7] and progress_end int32 [B,3]: the state after the last step (status 2: the
 *   state as given).  Passing them back as q_start, v_init, progress_init CONTINUES the rollout: k calls of max_steps m
 *   walk the dense path of one call of k m steps bit for bit -- the entry is a reactive controller that can be stepped.
 *   A row that comes in finished takes no step (steps 0) and is judged on T copies of q_start.
 *   No allocation, no scratch, no atomics; everything is enqueued on `stream` (capturable).  B == 0 launches nothing.    */
#define MPX_FOLLOW_MAX_POSES 64
#define MPX_FOLLOW_MAX_STEPS 4096
#define MPX_FOLLOW_BIT_MISS 8
#define MPX_FOLLOW_MISS_SHARE 0.9999f
#define MPX_FOLLOW_DEFAULT_DT 0.005f            /* gen_data.py:268 */
#define MPX_FOLLOW_DEFAULT_MAX_STEPS 1024
#define MPX_FOLLOW_DEFAULT_ATTRACT 144.0f
#define MPX_FOLLOW_DEFAULT_DAMPING 24.0f        /* critical for that stiffness */
#define MPX_FOLLOW_DEFAULT_REPEL 40.0f
#define MPX_FOLLOW_DEFAULT_LIMIT_GAIN 50.0f
#define MPX_FOLLOW_DEFAULT_LIMIT_BAND 0.1f
#define MPX_FOLLOW_DEFAULT_SPEED_LIMIT 1.6999f  /* the fabric config's cspace_speed_limit */
#define MPX_FOLLOW_DEFAULT_SWITCH_RADIUS 0.15f
#define MPX_FOLLOW_DEFAULT_SWITCH_STEPS 100     /* 0.5 s at dt */
#define MPX_FOLLOW_DEFAULT_FINAL_RADIUS 0.005f
#define MPX_FOLLOW_DEFAULT_FINAL_STEPS 800      /* 4 s at dt: gen_data.py:76, 278, 291-294 */
#define MPX_FOLLOW_DEFAULT_MISS_TOL 0.05f       /* gen_data.py:420 */
typedef struct mpx_follow_options { /* NULL options: the defaults above, lambda / step_clip the IK defaults, epsilon / substeps /
                                       check_margin / max_jerk the planner's, clearance 0, check_self 1 */
  float dt;                         /* > 0 [s]                                                          */
  int max_steps;                    /* 1 .. MPX_FOLLOW_MAX_STEPS: steps of this call                     */
  float attract, damping;           /* >= 0: gain on u, viscous damping                                  */
  float lambda, step_clip;          /* > 0: as in mpx_ik_options                                         */
  float repel;                      /* >= 0: gain on the obstacle gradient                               */
  float epsilon;                    /* > 0 [m]: width of the band in which an obstacle repels            */
  float clearance;                  /* [m], added to the radii in the obstacle term AND the verdict      */
  float limit_gain, limit_band;     /* >= 0: the joint-limit barrier and its width [rad]                 */
  float speed_limit;                /* > 0 [rad/s] per joint                                             */
  float switch_radius;              /* >= 0 [m]: advance to the next guide pose inside it                */
  int switch_steps;                 /* >= 1: ... or after this many steps on one pose                    */
  float final_radius;               /* >= 0 [m]: finished inside it of the last pose                     */
  int final_steps;                  /* >= 1: ... or after this many steps on the last pose               */
  int substeps;                     /* 1 .. 64: pieces per segment in the validity sweep                 */
  float check_margin;               /* >= 0 [m], as in mpx_plan_options                                  */
  float max_jerk;                   /* >= 0: largest third difference [rad]                              */
  int check_self;                   /* non-zero: self collisions invalidate                              */
  float miss_tol;                   /* >= 0 [m]                                                          */
} mpx_follow_options;
int mpx_franka_follow(const float *q_start, const float *poses, int B, int W, int T, float finger, const float *limits,
                      const float *sph_centers, const float *sph_radii, const int32_t *sph_link, int S,
                      const float *cub_inv_frames, const float *cub_dims, int M1, const float *cyl_inv_frames,
                      const float *cyl_radii, const float *cyl_heights, int M2, const float *v_init,
                      const int32_t *progress_init, const mpx_follow_options *options, float *path, float *arc,
                      int32_t *status, int32_t *bits, int32_t *steps, float *traj, float *traj_any, float *q_end,
                      float *v_end, int32_t *progress_end, mpx_stream_t stream);

/* A lazy probabilistic roadmap per problem for the FREE-FLYING GRIPPER in SE(3): where the reference's data generator plans
 * the end effector through the scene before it hands the pose path to the fabric (data_pipeline/gen_data.py:156-189,
 * plan_end_effector).  A STAND-IN for that OMPL planner, NOT a port of it and with no claim of parity with AIT*; "valid"
 * means free by this engine's sphere model, not by PyBullet's meshes.  One workgroup per problem; the result depends on the
 * inputs alone.  Its poses are an operand of mpx_franka_follow.
 *   start_pose, goal_pose [B,4,4] row-major right_gripper poses (mpx_franka_ik's targets; rows 0-2 are read); bounds
 *   [B,2,3] = lo, hi of the position box of each problem; the sphere table and the primitives exactly as for
 *   mpx_franka_roadmap (S <= 64, M1, M2 <= 64, zero-volume rows skipped).
 *   The gripper.  The rows of the sphere table with link id 9, 12 or 13 (panda_hand and the two fingertips; 20 of the standard
 *   56), the others are ignored.  From a right_gripper pose (R, p) a sphere centre c of link 9 has the hand-frame point
 *   h = c, of link 12 h = c + (0, finger, 0.0584f + 0.045f), of link 13 h = c + (0, -finger, 0.0584f + 0.045f); it sits at
 *   R (-h_x, -h_y, h_z - 0.1f) + p, the product as fma(R_i2, g_z, fma(R_i1, g_y, R_i0 g_x)) + p_i (mpx_franka_fk's fixed
 *   transforms from the hand to right_gripper, inverted).  R of a unit quaternion (x, y, z, w): R_00 = 1 - 2 (yy + zz),
 *   R_01 = 2 (xy - wz), R_02 = 2 (xz + wy), R_10 = 2 (xy + wz), R_11 = 1 - 2 (xx + zz), R_12 = 2 (yz - wx),
 *   R_20 = 2 (xz - wy), R_21 = 2 (yz + wx), R_22 = 1 - 2 (xx + yy), every product and sum rounded on its own.
 *   A pose is VALID by the planner's clause: no gripper sphere with sdf <= r_s + clearance + check_margin (the minimum over
 *   the live primitives; with S = 0 or no live primitive this test passes), and with check_self none of the origins of
 *   frames 9, 12, 13 -- R (0, 0, -0.1f) + p and R (0, -+finger, (0.0584f + 0.045f) - 0.1f) + p -- inside
 *   0.15 + 0.01 + check_margin of the base segment (mpx_franka_plan's self test on those frames).
 *   Nodes.  V = options->nodes, 2 <= V <= MPX_ROADMAP_MAX_NODES; a node is (p, q): position and unit quaternion (x, y, z, w).
 *   Node 0 is start_pose, node 1 goal_pose: p the last column, q by Shepperd's method -- with t = R_00 + R_11 + R_22 the
 *   branch is the first of (t, R_00, R_11, R_22) that is >= the other three; branch t: s = 2 sqrtf(1 + t), w = s / 4,
 *   x = (R_21 - R_12) / s, y = (R_02 - R_20) / s, z = (R_10 - R_01) / s; branch R_00: s = 2 sqrtf(1 + R_00 - R_11 - R_22),
 *   x = s / 4, w = (R_21 - R_12) / s, y = (R_01 + R_10) / s, z = (R_02 + R_20) / s; R_11 and R_22 by cyclic exchange -- then
 *   divided by its norm.  Node v >= 2: words 0-7 = Philox4x32-10(counter = {2v, GLOBAL problem id = env_offset + b,
 *   stream 17, 0}, key = seed) followed by the block with counter word 0 = 2v + 1, u_i = u01 of word i;
 *   p_k = fma(u_k, hi_k - lo_k, lo_k), k = 0..2; with sigma = +1 when dot(q_start, q_goal) >= 0, else -1,
 *   m_k = fma(u_3, sigma q_goal,k - q_start,k, q_start,k), raw_k = fma(orient_spread, fma(2, u_{4+k}, -1), m_k),
 *   q = raw / sqrtf(|raw|^2): orientations scatter about the start-goal arc (orient_spread = 0 puts them on it), they are
 *   NOT uniform on SO(3).  A drawn node with |raw|^2 < 2^-20 is invalid.  Every 4-vector dot and squared norm is
 *   fma(a_3, b_3, fma(a_2, b_2, fma(a_1, b_1, a_0 b_0))).
 *   status int32 [B]: 2 an endpoint pose has a non-finite entry in rows 0-2, lies outside bounds (NaN bounds fail) or is
 *   invalid (no search is done, rounds = 0); 0 a path was found; 1 none was.
 *   Edge (a,b), a < b, sigma_ab the sign of dot(q_a, q_b) as above:
 *   w = sqrtf(fma((2 rot_weight)^2, |q_b - sigma_ab q_a|^2, |p_b - p_a|^2)), each squared norm summed k ascending, the
 *   first square rounded on its own and the others fused, (2 rot_weight)^2 = (2 rot_weight) (2 rot_weight) in float32 (the
 *   same bits for (b,a)).  2 |q_a - sigma q_b| = 4 sin(theta / 4) ~ theta for a relative rotation theta: with rot_weight the
 *   largest lever arm of a sphere centre about the gripper origin (0.1172 m; default 0.12), w bounds how far any centre
 *   moves along the edge.  n = min(2^20, max(1, (int)ceilf(w / resolution))) pieces; interior pose i = 1 .. n-1 with
 *   f = (float)i / (float)n: p = fma(f, p_b - p_a, p_a), q = raw / sqrtf(|raw|^2), raw_k = fma(f, sigma_ab q_b,k - q_a,k,
 *   q_a,k) (nlerp).  The edge is BLOCKED exactly when an interior pose is invalid; an edge with w > connect_radius does not
 *   exist.
 *   Search: mpx_franka_roadmap's, statement for statement (Jacobi sweeps to a fixed point, u ascending with a strict "<",
 *   the untested edges of the round's path tested in full, at most max_rounds rounds), and its outputs path int32 [B,V],
 *   hops int32 [B], optional nodes [B,V,7] (p, then q), edge_state uint8 [B,V,V] (0 untested / 1 free / 2 blocked, the
 *   diagonal 1 for a valid node and 2 for an invalid one), rounds int32 [B].
 *   poses [B,W,4,4], 1 <= W <= MPX_FOLLOW_MAX_POSES: the start is not among them (the follower starts there).  With c_0 = 0,
 *   c_{i+1} = c_i + w_i summed in path order in float32 and s_t = ((float)(t+1) / (float)W) c_hops, pose t < W-1 lies on
 *   the last edge i with c_i <= s_t at f = min((s_t - c_i) / w_i, 1) (0 if w_i = 0), by the edge's nlerp taken in PATH
 *   order (from path node i toward i+1); rows 0-2 are [R | p] of that (p, q), R as above.  Rows 0-2 of pose W-1 are
 *   goal_pose's bit for bit.  Row 3 of every pose is (0, 0, 0, 1).  No smoothing: the follower switches poses inside its
 *   switch radius.  Rows with status != 0 are NaN (all 16 entries).
 *   No allocation, no scratch, no global atomics; everything is enqueued on `stream` (capturable).  B == 0 launches
 *   nothing.                                                                                                            */
#define MPX_GRIPPER_ROADMAP_DEFAULT_NODES 64
#define MPX_GRIPPER_ROADMAP_DEFAULT_RESOLUTION 0.01f   /* the smallest gripper sphere has radius 0.0108 */
#define MPX_GRIPPER_ROADMAP_DEFAULT_ROT_WEIGHT 0.12f   /* the lever arm 0.1172 m, rounded up            */
#define MPX_GRIPPER_ROADMAP_DEFAULT_ORIENT_SPREAD 0.5f
#define MPX_GRIPPER_ROADMAP_DEFAULT_MAX_ROUNDS 256     /* a round is cheap: 20 spheres per pose (profiles/gripper_roadmap_timing.md) */
typedef struct mpx_gripper_roadmap_options { /* NULL options: the defaults above, connect_radius +inf, check_margin
                                                MPX_PLAN_DEFAULT_CHECK_MARGIN, clearance 0, check_self 1 */
  int nodes;                                 /* 2 .. MPX_ROADMAP_MAX_NODES, start and goal included       */
  float resolution;                          /* > 0 [m]: the longest piece of an edge (the metric w)      */
  float rot_weight;                          /* > 0 [m/rad]: what a radian of rotation counts in w        */
  float orient_spread;                       /* >= 0: scatter of the drawn quaternions about the arc      */
  float connect_radius;                      /* [m], longer edges do not exist; +inf: the complete graph  */
  int max_rounds;                            /* >= 1: searches before giving up                           */
  float check_margin;                        /* >= 0 [m], as in mpx_plan_options                          */
  float clearance;                           /* [m], added to the radii                                   */
  int check_self;                            /* non-zero: the body column invalidates a pose              */
} mpx_gripper_roadmap_options;
int mpx_gripper_roadmap(const float *start_pose, const float *goal_pose, int B, int W, const float *bounds, float finger,
                        const float *sph_centers, const float *sph_radii, const int32_t *sph_link, int S,
                        const float *cub_inv_frames, const float *cub_dims, int M1, const float *cyl_inv_frames,
                        const float *cyl_radii, const float *cyl_heights, int M2,
                        const mpx_gripper_roadmap_options *options, uint64_t seed, int64_t env_offset, float *poses,
                        int32_t *status, int32_t *path, int32_t *hops, float *nodes, uint8_t *edge_state, int32_t *rounds,
                        mpx_stream_t stream);

/* TASK-ORIENTED gripper pose candidates: where the reference's scene generators draw a start or goal ON a scene's supports
 * (tabletop_environment.py:354-404, a point on a table top lifted onto the object it lies on, raised 1 to 12 cm, the gripper
 * pointing down; cubby_environment.py:440-549, a point inside a pocket, the gripper reaching in) and keep a draw when the
 * free-flying gripper is clear of the scene.  A restatement of those DISTRIBUTIONS, judged by this engine's sphere model
 * (the hand and fingertip spheres of the table, mpx_gripper_roadmap's gripper), not by PyBullet's meshes; the IK half of
 * the reference's test is mpx_franka_ik on the poses this entry returns.  One workgroup per problem, draw n on thread n;
 * the result depends on the inputs alone.
 *   support_boxes [B,NS,12]: centre (3), dims (3), UNIT quaternion w x y z (4), approach (1: the world yaw of the axis the
 *   gripper reaches along, volumes only), weight (1).  support_kind int32 [B,NS]: 0 padding, 1 a SURFACE (the box's top
 *   face, local z = +dims_z / 2), 2 a VOLUME (the box).  1 <= NS <= MPX_TASK_MAX_SUPPORTS.  exclude int32 [B] or NULL: the
 *   one support row of problem b that is not drawn from (-1 or out of range: none).  The sphere table and the primitives
 *   exactly as for mpx_gripper_roadmap (S <= 64, M1, M2 <= 64, zero-volume rows skipped); the primitives are ASSUMED to be
 *   rotated about the world z axis only: the top of a primitive is taken as -f_23 + size_z / 2, where f_23 is row 2,
 *   column 3 of its inverse frame (mpx_prim_frames: that entry is -centre_z exactly for such a rotation) and size_z the
 *   cuboid's third dim or the cylinder's height.
 *   Draw n = 0 .. N-1 (N = options->draws) of problem b: words 0-3 = Philox4x32-10(counter = {2n, GLOBAL problem id =
 *   env_offset + b, stream 18, options->role}, key = seed), words 4-7 the block with counter word 0 = 2n + 1; u_i = u01 of
 *   word i (top 24 bits / 2^24).  u_0 picks the support, u_1 u_2 u_3 the position, u_4 u_5 u_6 the orientation, u_7 is
 *   not used.  role 0 draws a start, role 1 a goal: two independent streams.
 *   1 Support.  w_s = weight_s where kind_s != 0, s != exclude_b and weight_s > 0, else 0 (NaN: 0); c_s = c_{s-1} + w_s
 *   in float32, s ascending; total = c_{NS-1}.  The draw's support is the first s with c_s > u_0 total.  total = 0:
 *   the problem has no live support and count = 0.
 *   2 Position.  With R_s the matrix of the support's quaternion (mpx_gripper_roadmap's R, its (x, y, z, w) read from
 *   (w, x, y, z) here) and l = ((u_1 - 0.5f) dims_x, (u_2 - 0.5f) dims_y, l_z): p = R_s l + centre, the product as
 *   fma(R_i2, l_z, fma(R_i1, l_y, R_i0 l_x)) + centre_i.  Volume: l_z = (u_3 - 0.5f) dims_z.  Surface: l_z = 0.5f dims_z;
 *   then every live primitive is visited in index order, cuboids before cylinders, and where its signed distance
 *   (mpx_cuboid_sdf / mpx_cylinder_sdf) to the CURRENT p is <= 0.01f, p_z becomes that primitive's top (the reference walks
 *   its objects the same way, against the already lifted point); then p_z += fma(1 - sqrtf(u_3), 0.11f, 0.01f): 1 to 12 cm,
 *   densest near the surface.
 *   3 Orientation.  Surface: roll = fma(u_4, pi/2, 3 pi/4), pitch = fma(u_5, pi/4, -pi/8), yaw = fma(u_6, pi, -pi/2)
 *   (roll in 3 pi/4 .. 5 pi/4, pitch +-pi/8, yaw +-pi/2), R = Rz(yaw) Ry(pitch) Rx(roll):
 *     R = [cy cp, cy sp sr - sy cr, cy sp cr + sy sr;  sy cp, sy sp sr + cy cr, sy sp cr - cy sr;  -sp, cp sr, cp cr],
 *   every product and sum rounded on its own, left to right (the convention is this entry's: geometrout's SO3.from_rpy is
 *   not restated anywhere in this project).  Volume: a = approach + fma(u_4, pi/2, -pi/4); the gripper's z axis is
 *   (cos a, sin a, 0), its x axis (0, 0, -1), y = z x x:  R = [0, -sin a, cos a;  0, cos a, sin a;  -1, 0, 0].  The
 *   constants are the float32 nearest to pi/2, pi/4, pi, 3 pi/4, pi/8; sines and cosines are float32 (within 2e-7).
 *   4 Verdict.  The draw is FREE when every entry of (R, p) is finite and the pose (R, p) is valid by
 *   mpx_gripper_roadmap's clause with check_margin 0: no gripper sphere with sdf <= r_s + clearance (with S = 0 or no live
 *   primitive this test passes), and with test_self none of the origins of frames 9, 12, 13 inside
 *   0.15 + 0.01 + self_margin of the base segment.
 *   Outputs, 1 <= C <= MPX_TASK_MAX_CANDIDATES: the first C free draws IN DRAW ORDER (an ordered compaction across the
 *   workgroup's waves: wave ballots and popcounts, no atomics).  count int32 [B] = min(C, free draws); for j < count:
 *   poses [B,C,4,4] row-major = [R | p; 0 0 0 1], draw int32 [B,C] = n (strictly ascending in j), support int32 [B,C] = s.
 *   Rows j >= count: all 16 pose entries NaN, draw = support = -1.
 *   Refused before any launch: draws outside 1 .. MPX_TASK_MAX_DRAWS, C or NS out of range, role not 0 or 1, clearance NaN,
 *   self_margin negative or NaN, S > 64, M1 or M2 > 64, env_offset + B > 2^32, B x C x 16 >= 2^31, NULL operands.  B == 0
 *   launches nothing.  One launch of B workgroups of 128 threads on grid.x, like the other per-problem entries (no slab
 *   walk: grid.x reaches 2^31 - 1); 9.3 kB of LDS, no scratch, no allocation, no global atomics; enqueued on `stream`
 *   (capturable).                                                                                                        */
#define MPX_TASK_MAX_DRAWS 128
#define MPX_TASK_MAX_CANDIDATES 16
#define MPX_TASK_MAX_SUPPORTS 64
#define MPX_TASK_DEFAULT_DRAWS 100 /* the reference's tries per candidate */
typedef struct mpx_task_candidates_options { /* NULL options: draws MPX_TASK_DEFAULT_DRAWS, clearance 0, test_self 1,
                                                self_margin 0, role 0 */
  int draws;                                 /* 1 .. MPX_TASK_MAX_DRAWS: one thread each                       */
  float clearance;                           /* [m], added to the radii                                        */
  int test_self;                             /* non-zero: the body column rejects a draw                       */
  float self_margin;                         /* >= 0 [m], added to the self distances                          */
  int role;                                  /* 0 a start, 1 a goal: counter word 3 of every draw              */
} mpx_task_candidates_options;
int mpx_task_candidates(const float *support_boxes, const int32_t *support_kind, int B, int NS, const int32_t *exclude, int C,
                        float finger, const float *sph_centers, const float *sph_radii, const int32_t *sph_link, int S,
                        const float *cub_inv_frames, const float *cub_dims, int M1, const float *cyl_inv_frames,
                        const float *cyl_radii, const float *cyl_heights, int M2,
                        const mpx_task_candidates_options *options, uint64_t seed, int64_t env_offset, float *poses,
                        int32_t *draw, int32_t *support, int32_t *count, mpx_stream_t stream);

/* SCENES drawn on the device: the distributions of the host generators (mpinets_amd/scenes.py: _tabletop, _cubby, _dresser,
 * themselves restatements of the reference's tabletop_environment.py:215-324, cubby_environment.py:62-74 and
 * dresser_environment.py:198-222) with the supports make_task_scenes reads off them, every scene a function of
 * (seed, scene id, kind, M1, M2, S) alone: a shard generates its own rows and nothing else.  A second SOURCE of scenes, not
 * a port of the host's stream: numpy's PCG64 is sequential, these draws are counter-keyed, so the same seed gives other
 * scenes of the same distribution.  One wave per scene, a lane per primitive slot, four scenes per workgroup.
 *   scene_kind int32 [B]: 0 tabletop, 1 cubby, 2 dresser; any other code: an EMPTY scene (all padding, no supports).
 *   scene_ids int64 [B] or NULL: the id of scene b (its low 32 bits are used); NULL: id = scene_offset + b.
 *   3 <= M1 <= 64, 0 <= M2 <= 64.  support_boxes and support_kind both NULL with S == 0 (make_scenes' form), or both given
 *   with 1 <= S <= MPX_TASK_MAX_SUPPORTS.
 *   Outputs, make_task_scenes' arrays: cuboid_centers [B,M1,3], cuboid_dims [B,M1,3], cuboid_quats [B,M1,4] (w x y z),
 *   cylinder_centers [B,M2,3], cylinder_radii [B,M2,1], cylinder_heights [B,M2,1], cylinder_quats [B,M2,4]; support_boxes
 *   [B,S,12] = centre (3), dims (3), quaternion w x y z (4), approach, weight; support_kind int32 [B,S] (0 padding,
 *   1 surface, 2 volume: mpx_task_candidates' operands).  EVERY element is written: live rows form a prefix of each array,
 *   the rows behind them are PADDING = zero centre, zero dims / radius / height, quaternion (1, 0, 0, 0), and for a
 *   support approach 0, weight 0, kind 0.  Every cylinder quaternion is (1, 0, 0, 0); every quaternion of a live row is
 *   (qw, 0, 0, qz): the scenes are rotated about the world z axis only.
 *   Draws.  word j of (item, block) = word j of Philox4x32-10(counter = {item, scene id, stream 19, block}, key = seed);
 *   u(item, j) = u01 of word j of block 0 for j = 0..3 and of word j - 4 of block 1 for j = 4..7 (top 24 bits / 2^24).
 *   Item 0 carries the scene's parameters, item k + 1 object or plate k.  A threshold compares u with the float32 constant
 *   written; an integer draw from word x is  (((x >> 8) * n) >> 24)  in integer arithmetic.  All arithmetic is float32, each
 *   operation rounded on its own in the order written, fma(a, b, c) = a b + c rounded once only where it is written;
 *   decimal constants are the nearest float32; pi/2 = 1.57079632679489661923f, pi/18 = 0.17453292519943295f,
 *   pi/9 = 0.3490658503988659f, pi/6 = 0.52359877559829887f, 2 pi/3 = 2.0943951023931953f.  sin and cos are float32
 *   (within 2e-7).  The quaternion of a yaw is q(yaw) = (cos(0.5f yaw), 0, 0, sin(0.5f yaw)); with c = cos(yaw), s = sin(yaw)
 *   a local point (lx, ly, lz) lies at  W(l) = ((c lx - s ly) + ox, s lx + c ly, lz + oz)  for the kind's origin (ox, oz).
 *   TABLETOP (kind 0), with u_j = u(0, j):
 *     h = 0 if u_0 < 0.35f else u_1 0.4f;  x0 = fma(u_2, 0.1f, 0.275f);  x1 = fma(u_3, 0.1f, 1.275f);
 *     w = fma(u_4, 0.15f, 1.5f);  a side table stands iff u_5 < 0.5f, at side = -1 if u_6 < 0.5f else +1;
 *     K = 3 + integer draw (n = 12) from word 3 of block 1: 3 .. 14 objects.
 *     Cuboid 0, the front table: centre ((x0 + x1) 0.5f, 0, h - 0.025f), dims (x1 - x0, w, 0.05f).  Cuboid 1, with a side
 *     table: centre (0, side fma(w, 0.25f, 0.45f), h - 0.025f), dims (0.9f, w 0.5f, 0.05f).  The next cuboid, the mount
 *     table: centre (-0.35f, 0, -0.025f), dims (0.6f, 0.6f, 0.05f).  T = 2 or 3 tables, identity quaternions.
 *     Object k = 0 .. K-1, with v_j = u(k + 1, j):  lo = x0 + 0.1f, px = fma(v_0, (x1 - 0.1f) - lo, lo);
 *     hw = w 0.5f - 0.1f, py = fma(v_1, hw + hw, -hw);  it DREW a cylinder iff v_2 < 0.3f (v_3 is not used).
 *     Slots, the host loop's rule without the loop: object k IS a cylinder when it drew one and fewer than M2 objects before
 *     it did; its row is the number of those.  Otherwise it is a cuboid candidate (an overflowing cylinder draw included),
 *     kept when r = the number of cuboid candidates before it satisfies T + r < M1, in row T + r; otherwise dropped.
 *     Cylinder: radius fma(v_4, 0.1f, 0.05f), height hh = fma(v_5, 0.3f, 0.05f), centre (px, py, fma(hh, 0.5f, h)).
 *     Cuboid: dims (fma(v_4, 0.1f, 0.05f), fma(v_5, 0.1f, 0.05f), dz = fma(v_6, 0.3f, 0.05f)), centre (px, py,
 *     fma(dz, 0.5f, h)), quaternion q(v_7 pi/2).
 *     Supports: row 0 the front table, row 1 the side table where it stands (the first S of them): SURFACES, the cuboid's
 *     centre, dims and quaternion copied, approach 0, weight = dims_x dims_y.  The mount table is not a support.
 *   CUBBY (kind 1), with u_j = u(0, j):  t = fma(u_0, 0.02f, 0.01f), W = fma(u_1, 0.4f, 0.7f), H = fma(u_2, 0.4f, 0.5f),
 *     D = fma(u_3, 0.15f, 0.2f), ox = fma(u_4, 0.25f, 0.55f), oz = fma(u_5, 0.2f, 0.1f), yaw = fma(u_6, pi/9, -pi/18);
 *     with hH = H 0.5f, hW = W 0.5f, ht = t 0.5f the first min(7, M1) of the plates (local centre; dims), all q(yaw), at W(l):
 *       0 (0, 0, 0; D, W, t)   1 (0, 0, H; D, W, t)   2 (0, 0, hH; D, W, t)   3 (0, -hW, hH; D, t, H)   4 (0, hW, hH; D, t, H)
 *       5 (0, 0, hH; D, t, H)   6 (D 0.5f, 0, hH; t, W, H).
 *     Supports: the first min(4, S) pockets p = 2 zi + yi, VOLUMES:  (z0, z1) = (ht, hH - ht) for zi = 0, (hH + ht, H - ht)
 *     for zi = 1;  (y0, y1) = (-hW + ht, -ht) for yi = 0, (ht, hW - ht) for yi = 1;  centre W(-(t 0.25f), (y0 + y1) 0.5f,
 *     (z0 + z1) 0.5f), dims (D - ht, y1 - y0, z1 - z0), q(yaw), approach 0, weight 1.
 *   DRESSER (kind 2), with u_j = u(0, j):  W = fma(u_0, 0.4f, 0.8f), D = fma(u_1, 0.2f, 0.2f), H = fma(u_2, 0.3f, 0.55f),
 *     ox = fma(u_3, 0.2f, 0.55f), oz = 0, yaw = fma(u_4, 2 pi/3, pi/6);  n = min(M1, 12 + integer draw (n = 29) from word 1
 *     of block 1): 12 .. 40 plates before the min;  rows = the smallest integer r with r r >= n;  wc = W / (float)rows,
 *     hc = H / (float)rows.  Plate i = 0 .. n-1 in cell (ri, ci) = (i / rows, i mod rows), depth jitter
 *     j = fma(u(i + 1, 0), 0.04f, -0.02f):  centre W(fma((float)ci + 0.5f, wc, -(W 0.5f)), j, ((float)ri + 0.5f) hc), dims
 *     (wc 0.95f, D, hc 0.2f), q(yaw).  Supports: one VOLUME per plate, the first min(S, n): the plate's centre with local z
 *     ((float)ri + 0.8f) hc, dims (wc 0.95f, D, hc 0.4f), q(yaw), weight 1, approach = yaw - pi/2.  (The host picks the sense
 *     of the depth axis with a positive world-x component, yaw + pi/2 where sin(yaw) < 0; the drawn yaw lies in
 *     (pi/6, 5 pi/6), its sine is positive, so the approach is yaw - pi/2 ALWAYS and the kernel does not test it.)
 *   An output is at most eight rounded operations from its uniforms plus one sine or cosine on a lever arm below 1 m:
 *   within about 1.2e-6 of exact arithmetic at the largest coordinate, 2 m.  The discrete decisions (thresholds, K, n, rows,
 *   slots) are exact.
 *   Refused before any launch: M1 outside 3 .. 64, M2 outside 0 .. 64, one support pointer without the other, S != 0 without
 *   them or outside 1 .. MPX_TASK_MAX_SUPPORTS with them, scene_offset < 0, scene_offset + B > 2^32 (checked with scene_ids
 *   too), B < 0; then B == 0 launches nothing; then a NULL scene_kind or primitive pointer (M2 == 0 excuses the four cylinder
 *   pointers), or a cuboid_quats, cylinder_quats or support_boxes that is not 16-byte aligned (their rows are stored as
 *   float4).  ceil(B / 4) workgroups of 256 threads on grid.x; no LDS (the slot compaction is two wave ballots and
 *   popcounts), no scratch, no allocation, no global atomics; enqueued on `stream` (capturable).                        */
int mpx_scene_generate(const int32_t *scene_kind, const int64_t *scene_ids, int B, int M1, int M2, int S, uint64_t seed,
                       int64_t scene_offset, float *cuboid_centers, float *cuboid_dims, float *cuboid_quats,
                       float *cylinder_centers, float *cylinder_radii, float *cylinder_heights, float *cylinder_quats,
                       float *support_boxes, int32_t *support_kind, mpx_stream_t stream);

/* SCENES AS THE REFERENCE BUILDS THEM, drawn on the device: kind 3 the tabletop of setup_tables + place_objects +
 * random_object (tabletop_environment.py:129-153, 215-324, 406-441; K from gen_data.py:618), kind 4 the cubby of
 * Cubby.__init__ / .cuboids / .support_volumes (cubby_environment.py:62-431), kind 5 the merged cubby
 * (MergedCubbyEnvironment, :660-704): that cubby with the plates between two pockets removed.  Restated from those lines,
 * not copied.  geometrout is not in this tree: that its Cuboid.random, Cylinder.random and sample_volume draw uniformly
 * between the bounds they are given is RECALLED, not pinned.  A new entry beside mpx_scene_generate, which it leaves as it
 * is: operands, outputs, padding, keying and the Draws paragraph are that entry's, with these differences.
 *   scene_kind int32 [B]: rows whose code is not 3, 4 or 5 are left UNTOUCHED (no element of theirs is written): a mixed
 *   batch is mpx_scene_generate followed by this entry on the same arrays.  Of a row with code 3, 4 or 5 every element is
 *   written.  7 <= M1 <= 64 (the cubby's plates), 0 <= M2 <= 64.
 *   merge_pockets int32 [B,2] or NULL, read for kind 5 alone: the pocket pair (a, b) of scene b.  NULL: the scene draws its
 *   pair.  (-1, -1): unmerged.  Anything else that is not a pair of DISTINCT pockets in 0 .. 3 is UNMERGED too (the operand
 *   lives on the device, a launch cannot refuse it; scenes.make_scenes_device refuses it where it is handed host values).
 *   Every scene is a function of (seed, scene id, kind, M1, M2, S, pair) alone; kinds 4 and 5 with one id and seed are the
 *   same cubby.  Item 0 has FOUR blocks: u_j = u(0, j), j = 0 .. 15, is u01 of word j mod 4 of block j / 4.
 *   TABLETOP (kind 3):  h = 0 if u_0 < 0.35f else u_1 0.4f.  Every table is a solid block from z = -0.02 to h: centre z
 *     tz = (h - 0.02f) 0.5f, dim z td = h + 0.02f.  Front table: fx0 = fma(u_2, 0.1f, 0.275f), fx1 = fma(u_3, 0.1f, 1.275f),
 *     fy1 = fma(u_4, 0.15f, 1.5f); a side table stands iff u_5 < 0.5f; fy0 = fma(u_6, 0.25f, -1.0f) with it (-1 .. -0.75),
 *     else fma(u_6, 0.2f, -0.75f) (-0.75 .. -0.55).  Dx = fx1 - fx0, Dy = fy1 - fy0, ty = fma(u_7, 0.1f, 0.55f) Dy.
 *       front TASK table: centre ((fx0 + fx1) 0.5f, fma(ty, 0.5f, fy0), tz), dims (Dx, ty, td);
 *       front FREE table: centre ((fx0 + fx1) 0.5f, (fy1 + (fy0 + ty)) 0.5f, tz), dims (Dx, Dy - ty, td).
 *     Side table (:272-303): sy1 = fma(u_8, 0.05f, -0.325f), length L = u_9 1.375f, sdx = L fma(u_10, 0.1f, 0.55f),
 *     SDy = sy1 - fy0; it spans x from fx0 - L to fx0 and y from fy0 to sy1, split along x:
 *       side TASK table (anchored at x max): centre (fx0 - sdx 0.5f, (sy1 + fy0) 0.5f, tz), dims (sdx, SDy, td);
 *       side FREE table: centre (((fx0 - L) + (fx0 - sdx)) 0.5f, (sy1 + fy0) 0.5f, tz), dims (L - sdx, SDy, td).
 *     Mount table (:306-324): mcx = fma(u_11, 0.04f, -0.02f), mcy = fma(u_12, 0.04f, -0.02f); centre (mcx, mcy, -0.01f),
 *     dims (2 (fx0 - mcx), 2 (mcy - sy1) with a side table else fma(u_13, 0.04f, 0.9f), 0.02f).  The reference draws side_x
 *     (:283), xdim (:315) and ydim (:321) and uses none of them: they are DROPPED, no uniform stands for them (u_14 is not
 *     used).  K = 3 + integer draw (n = 12) from word 3 of block 3: 3 .. 14 objects.
 *     Cuboid rows, the reference's `obstacles` order: task tables, free tables, mount table, objects -- with a side table
 *     front task, side task, front free, side free, mount (T = 5), without front task, front free, mount (T = 3); identity
 *     quaternions.  Supports: the task tables, front then side (the first S): SURFACES, the cuboid's centre, dims and
 *     quaternion copied, approach 0, weight = dims_x dims_y.  Free tables and the mount table are not supports.
 *     Candidates c = 0 .. 10 K - 1, points on the task tables' top faces, v_j = u(c + 1, j), j = 0 .. 7 (two blocks): with
 *     A0 = Dx ty and A1 = sdx SDy (0 without a side table) the point lies on the side task table iff one stands and
 *     v_0 (A0 + A1) >= A0 (probability proportional to the top face's area), at x = fma(v_1, sdx, fx0 - sdx),
 *     y = fma(v_2, SDy, fy0); else on the front task table at x = fma(v_1, Dx, fx0), y = fma(v_2, ty, fy0).
 *     The walk (place_objects): candidates in order while fewer than K objects are placed.  For a placed object i and
 *     (dx, dy) = (x - x_i, y - y_i) the FOOTPRINT DISTANCE is, for a cylinder, sqrtf(fma(dx, dx, dy dy)) - radius_i; for a
 *     cuboid with (ci, si) = (cos, sin) of its yaw: lx = fma(ci, dx, si dy), ly = fma(ci, dy, -(si dx)),
 *     qx = |lx| - 0.5f dims_x, qy = |ly| - 0.5f dims_y, ex = max(qx, 0), ey = max(qy, 0),
 *     d = sqrtf(fma(ex, ex, ey ey)) + min(max(qx, qy), 0).  The candidate is ACCEPTED iff every d_i > 0.05f.  This 2-D
 *     test is the reference's 3-D sdf test: all objects stand on the table top, the candidate lies in the plane of their
 *     bottom faces, so its offset along an object's axis is exactly the half height and contributes nothing; outside the
 *     footprint the 3-D distance is the 2-D one, inside it both are <= 0 and the candidate is rejected either way.
 *     m = the least d_i (1000 with nothing placed), xm = min(m, 0.15f), span = xm - 0.05f (> 0).  The object is a cylinder
 *     iff v_3 < 0.3f: radius fma(v_4, span, 0.05f), height hh = fma(v_5, 0.3f, 0.05f), centre (x, y, fma(hh, 0.5f, h)).
 *     Otherwise a cuboid: dims (fma(v_4, span, 0.05f), fma(v_5, span, 0.05f), dz = fma(v_6, 0.3f, 0.05f)), yaw v_7 pi/2,
 *     quaternion q(yaw), centre (x, y, fma(dz, 0.5f, h)).  Cylinders fill rows 0, 1, .. of their arrays, cuboids rows T,
 *     T + 1, .. in the order accepted.  OVERFLOW: an accepted cylinder with M2 cylinders placed, or an accepted cuboid whose
 *     row would be M1, gets no row, does not count towards K and does not block later candidates; the walk goes on.
 *   CUBBY (kind 4) and MERGED CUBBY (kind 5):  left = fma(u_0, 0.2f, 0.6f), right = fma(u_1, 0.2f, -0.8f),
 *     bottom = fma(u_2, 0.2f, 0.1f), front = fma(u_3, 0.2f, 0.45f), back = front + fma(u_4, 0.4f, 0.15f),
 *     top = fma(u_5, 0.2f, 0.6f), mz = fma(u_6, 0.2f, 0.35f) (the shelf's height), my = fma(u_7, 0.2f, -0.1f) (the centre
 *     wall's y), t = fma(u_8, 0.02f, 0.01f) (both plate thicknesses too), yaw = fma(u_9, pi/9, -pi/18): the reference's twelve.
 *     The plates are rotated about the vertical axis through the cabinet's centre (px, py) = ((front + back) 0.5f,
 *     (left + right) 0.5f): a local point l lies at  W(l) = ((c ax - s ay) + px, (s ax + c ay) + py, lz)  with ax = lx - px,
 *     ay = ly - py, (c, s) = (cos, sin) of yaw, every product, difference and sum rounded on its own.  With
 *     pz = (top + bottom) 0.5f, Dd = back - front, Wd = left - right, Hd = (top - bottom) + t the seven plates in the
 *     reference's order (local centre; dims), all q(yaw):
 *       0 back (back, py, top 0.5f; t, Wd, top: it reaches the floor)   1 bottom (px, py, bottom; Dd, Wd, t)
 *       2 top (px, py, top; Dd, Wd, t)   3 right (px, right, pz; Dd, t, Hd)   4 left (px, left, pz; Dd, t, Hd)
 *       5 centre wall (px, my, pz; Dd, t, Hd)   6 middle shelf (px, py, mz; Dd, Wd, t).
 *     The reference leaves the centre wall or the shelf out where isclose(position, 0): an event of measure zero in these
 *     ranges for the wall and impossible for the shelf; a cubby here ALWAYS has seven plates.
 *     Supports, unmerged: the four pockets p = 2 level + side of support_volumes' last branch in its order, level 0 the top
 *     (z from mz to top; level 1 from bottom to mz), side 0 the +y side (y from my to left; side 1 from right to my):
 *     VOLUMES, centre W(px, (ya + yb) 0.5f, (za + zb) 0.5f), dims (Dd, yb - ya, zb - za), q(yaw), approach 0, weight 1.
 *     Merge, by MergedCubbyEnvironment's rule for a pair (a, b) of distinct pockets: the middle shelf goes when a and b lie
 *     on different levels (a >> 1 != b >> 1), the centre wall when they lie on different sides (a & 1 != b & 1).  A removed
 *     plate is DROPPED and the later rows move up (5 or 6 live plates): this tree's padding is the all-zero row and not
 *     every consumer masks a cuboid with a single zero dim.  The reference instead keeps a zero-thickness cuboid that its
 *     own consumers mask.  Supports become the matching branch of support_volumes, the whole extents taking the place of the
 *     removed plate's position: both gone: ONE volume (y right .. left, z bottom .. top), every pocket p maps to support 0;
 *     the wall alone gone: [top row, bottom row], p maps to p >> 1; the shelf alone gone: [left (+y) column, right column],
 *     p maps to p & 1.  Without merge_pockets the pair is the i-th of (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), i = integer draw
 *     (n = 6) from word 0 of block 3: one more uniform, which the cubby's own parameters do not read.
 *   The longest chain is a rotated plate's or pocket's x or y: a parameter (one fma; back: two), px or py (two more), ax or
 *   ay (one), two products, their sum, + p: at most ten rounded operations, each within 0.5 ulp (6e-8 below 1 m, 1.2e-7 at
 *   2 m), plus a float32 sine and cosine within 2e-7 on a lever arm below 0.45 m: within about 1.4e-6 of exact arithmetic.
 *   The tabletop's objects are at most five operations from their uniforms; its span = min(m, 0.15f) - 0.05f carries the
 *   error of m (a dozen operations on magnitudes below 2 m and a square root), scaled by a uniform below 1.  Discrete
 *   decisions that read a uniform alone are exact; the candidate's table and the accept test compare computed floats.
 *   Refused before any launch: as mpx_scene_generate, with M1 outside 7 .. 64.  ceil(B / 4) workgroups of 256 threads on
 *   grid.x, one wave per scene: every lane draws three candidates up front, the accept walk of at most 140 steps holds the
 *   placed objects one per lane and combines the verdict with a ballot and the least distance with four lane exchanges.
 *   No LDS, no scratch, no allocation, no atomics; enqueued on `stream` (capturable).                                   */
int mpx_scene_generate_reference(const int32_t *scene_kind, const int64_t *scene_ids, const int32_t *merge_pockets, int B, int M1,
                                 int M2, int S, uint64_t seed, int64_t scene_offset, float *cuboid_centers, float *cuboid_dims,
                                 float *cuboid_quats, float *cylinder_centers, float *cylinder_radii, float *cylinder_heights,
                                 float *cylinder_quats, float *support_boxes, int32_t *support_kind, mpx_stream_t stream);

/* ---- planning against a point cloud: a truncated distance field, its sampler, the planner that reads it -------------
 * One grid for the whole batch (a host struct, read before the launch): node (i,j,k), 0 <= i < nx etc., sits at
 *   (fma((float)i, h, lo[0]), fma((float)j, h, lo[1]), fma((float)k, h, lo[2]))  in float32.
 * lo and trunc finite, h finite and > 0, trunc > 0, 2 <= nx, ny, nz <= MPX_FIELD_MAX_SIDE, nx*ny*nz <= MPX_FIELD_MAX_NODES;
 * anything else is refused before a launch.                                                                            */
#define MPX_FIELD_MAX_SIDE 1024
#define MPX_FIELD_MAX_NODES (1 << 24)
typedef struct mpx_field_grid {
  float lo[3];    /* world position of node (0,0,0) */
  float h;        /* node spacing [m], > 0 */
  int nx, ny, nz; /* nodes per axis */
  float trunc;    /* > 0: the field saturates here */
} mpx_field_grid;

/* field [B,nz,ny,nx] float32 (x fastest) = the distance of every node to the nearest point of environment b's cloud, cut
 * at grid->trunc.  The cloud is addressed exactly as for mpx_franka_cloud_collision (strides in floats, point stride >= 3,
 * `xyz[:, 2048:6144, :3]` of the slab read in place; counts optional int32 [B], clamped to [0, N] on the device, NULL: N).
 *   best  = +inf; over the existing rows whose three coordinates are finite:
 *           best = min(best, d2),  d2 = fma(dz,dz, fma(dx,dx, dy*dy)) with dx = node.x - p.x, dy, dz likewise (float32: the
 *           library's one squared distance, the argument order of mpx_franka_cloud_collision with the node as the centre)
 *   field = fminf(sqrtf(best), trunc)          (an environment without a usable row: trunc everywhere)
 * A minimum does not depend on the order of its operands and nothing is accumulated, so the result depends on the inputs
 * alone: not on the launch shape, not on the order in which points are staged.  A workgroup owns a brick of
 * MPX_FIELD_BRICK^3 nodes and drops the points outside the brick's box inflated by more than trunc: a dropped point is
 * farther than trunc from every node of the brick, so it could only have produced a value that the fminf replaces by
 * trunc.  No allocation, no atomics on global memory, no scratch; B == 0 launches nothing.                              */
#define MPX_FIELD_BRICK 8
int mpx_cloud_field_build(const float *cloud, int64_t cloud_batch_stride, int cloud_point_stride, int N,
                          const int32_t *counts, int B, const mpx_field_grid *grid, float *field, mpx_stream_t stream);

/* Trilinear interpolant of the node values and its analytic derivative at points [B,P] (point p of environment b = the
 * three floats at points + b*points_batch_stride + p*points_point_stride, strides in floats, point stride >= 3).
 * dist [B,P]; grad [B,P,3] optional (NULL: not computed).  All in float32:
 *   inv_h = 1.0f / h (once, on the host);  u = (x - lo[0]) * inv_h, v and w likewise for y and z
 *   INSIDE: 0 <= u <= nx-1 and 0 <= v <= ny-1 and 0 <= w <= nz-1 (a NaN or infinite coordinate fails).  Not inside:
 *   dist = trunc, grad = 0 -- the caller sizes the grid to the workspace.
 *   i0 = min((int)floorf(u), nx-2), fx = u - (float)i0 (fx = 1 only on the last node of an axis); j0, fy, k0, fz likewise.
 *   Corners c[z][y][x] = field[b, k0+z, j0+y, i0+x]; every lerp is lerp(f, a, b) = fma(f, b - a, a), so f = 0 returns a
 *   bit for bit: a sample whose u, v, w are exact node indices below the last returns the node's value.
 *   along x: a[z][y] = lerp(fx, c[z][y][0], c[z][y][1]);  along y: e[z] = lerp(fy, a[z][0], a[z][1]);
 *   dist = lerp(fz, e[0], e[1])
 *   grad.x = inv_h * lerp(fz, lerp(fy, X[0][0], X[0][1]), lerp(fy, X[1][0], X[1][1])),  X[z][y] = c[z][y][1] - c[z][y][0]
 *   grad.y = inv_h * lerp(fz, a[0][1] - a[0][0], a[1][1] - a[1][0])
 *   grad.z = inv_h * (e[1] - e[0])
 * A SURFACE field: unsigned, no inside; the gradient is that of the interpolant (discontinuous across cell faces, not of
 * unit length).  The result depends on the inputs alone.                                                               */
int mpx_cloud_field_sample(const float *field, const mpx_field_grid *grid, int B, const float *points,
                           int64_t points_batch_stride, int points_point_stride, int P, float *dist, float *grad,
                           mpx_stream_t stream);

/* mpx_franka_plan against a POINT CLOUD: the same planner -- candidates (Philox stream 14), L, M, the clamp, endpoints
 * bit-equal, iterations = 0, the jerk bit, the self bit, the lowest valid candidate, choice, NaN rows on status != 0,
 * options with the same defaults and the same refusals -- with these differences:
 *   Environment term of one iteration.  D, n = mpx_cloud_field_sample's dist and grad of `field` [B,nz,ny,nx] (built by
 *   mpx_cloud_field_build on `grid`) at the sphere centre x_s;  d_s = ((D - point_radius) - r_s) - clearance;  a sphere
 *   with D >= trunc is saturated and contributes nothing (so does a centre outside the grid);  c'(d) as for
 *   mpx_franka_plan;  n_s = n as sampled, not normalised.  field == NULL: no environment term.
 *   Environment validity (bit 0 of all_status).  Candidate k is invalid exactly when mpx_franka_cloud_collision flags its
 *   refined configurations [B,R,7], R = (T-1) substeps + 1 (r = t substeps + i, the same fma), against environment b's
 *   cloud (cloud, strides, N, counts: as there) with this point_radius and clearance = options->clearance +
 *   options->check_margin summed in float32: that entry itself is called, once per candidate, flags only.  The field
 *   steers the optimiser and never judges.  cloud == NULL or N == 0 or S == 0: no environment test.
 *   status 2: mpx_franka_plan's rule (an endpoint not finite, outside the limits, self hit with check_self), the
 *   environment test being that call on the two endpoints [B,2,7].
 * scratch: device memory, 16-byte aligned, at least mpx_franka_plan_cloud_scratch(B, T, candidates, substeps) bytes (-1 for
 * sizes the planner refuses), owned by the caller, free when the stream has passed the call.  No allocation; every step
 * is enqueued on `stream` (a memset of the flags, the optimise kernel, candidates + 1 flag calls, a select kernel).
 * S <= 64, point_radius >= 0; B == 0 launches nothing.                                                                 */
int64_t mpx_franka_plan_cloud_scratch(int B, int T, int candidates, int substeps);
int mpx_franka_plan_cloud(const float *q_start, const float *q_goal, int B, int T, float finger, const float *limits,
                          const float *sph_centers, const float *sph_radii, const int32_t *sph_link, int S,
                          const float *field, const mpx_field_grid *grid, const float *cloud, int64_t cloud_batch_stride,
                          int cloud_point_stride, int N, const int32_t *counts, float point_radius,
                          const mpx_plan_options *options, uint64_t seed, int64_t env_offset, float *traj, int32_t *status,
                          int32_t *choice, float *all_traj, int32_t *all_status, void *scratch, int64_t scratch_bytes,
                          mpx_stream_t stream);

/* mpx_franka_plan_cloud with caller-supplied candidates, on the terms of mpx_franka_plan_seeded: seeds [B,Ks,T,7], Ks >= 0,
 * candidates + Ks <= MPX_PLAN_MAX_CANDIDATES.  Candidates 0 .. K-1 (K = options->candidates) are drawn and optimised exactly
 * as by mpx_franka_plan_cloud; candidate K + i starts from seeds[b,i]: its interior waypoints clamped into the limits,
 * waypoints 0 and T-1 replaced by q_start / q_goal; L stays the straight line for every candidate.  A seed with an entry
 * that is not finite is not a candidate: its all_traj rows are NaN and its all_status is 7 (its wave runs from the line,
 * so every scratch row the flag calls read is finite).  Iterations, the flag calls (K + Ks + 1 of them), the bits, "the
 * LOWEST valid candidate" and status 2 are mpx_franka_plan_cloud's; all_traj is [B,K+Ks,T,7], all_status [B,K+Ks], choice
 * counts over K + Ks.  Hence: with Ks = 0 (or seeds == NULL and Ks = 0) every output is bit-equal to
 * mpx_franka_plan_cloud's (it is that launch); with any Ks candidates 0 .. K-1 are bit-equal, and a row
 * mpx_franka_plan_cloud solves comes back identical.  scratch: at least mpx_franka_plan_cloud_scratch(B, T, candidates + Ks,
 * substeps) bytes.  Ks > 0 with seeds == NULL is refused.                                                               */
int mpx_franka_plan_cloud_seeded(const float *q_start, const float *q_goal, int B, int T, float finger, const float *limits,
                                 const float *sph_centers, const float *sph_radii, const int32_t *sph_link, int S,
                                 const float *field, const mpx_field_grid *grid, const float *cloud,
                                 int64_t cloud_batch_stride, int cloud_point_stride, int N, const int32_t *counts,
                                 float point_radius, const mpx_plan_options *options, uint64_t seed, int64_t env_offset,
                                 const float *seeds, int Ks, float *traj, int32_t *status, int32_t *choice, float *all_traj,
                                 int32_t *all_status, void *scratch, int64_t scratch_bytes, mpx_stream_t stream);

/* mpx_franka_roadmap against a POINT CLOUD, read through its distance field: the global half in front of
 * mpx_franka_plan_cloud_seeded.  Every clause of mpx_franka_roadmap's contract holds unchanged -- the nodes (Philox stream
 * 16 keyed by (seed, GLOBAL problem id, node): the same seed gives the same nodes as mpx_franka_roadmap), the edge pieces,
 * the Jacobi sweeps, the rounds, the statuses, path / hops / nodes / edge_state / rounds, the one-edge path that is the
 * planner's line bit for bit, resampling and the (1/4, 1/2, 1/4) passes, NaN rows where status != 0 -- except what makes a
 * configuration INVALID:
 *   with check_self, mpx_franka_plan's self test with check_margin fails; or
 *   some collision sphere s is BLOCKED.  Its centre c is that of mpx_franka_fk's chain in float32; (inside, D) =
 *   mpx_cloud_field_sample's INSIDE and dist of `field` [B,nz,ny,nx] (environment b of THIS call, built by
 *   mpx_cloud_field_build on `grid`) at c.  Blocked: c is inside the grid AND D < trunc AND
 *       d <= check_margin + field_slack,   d = ((D - point_radius) - r_s) - clearance
 *   (d is mpx_franka_plan_cloud's own expression, in that order, in float32; the right-hand side is summed once on the host
 *   in float32).  A centre outside the grid, or where the field is saturated, counts as FREE: the field knows nothing
 *   there, which is mpx_franka_plan_cloud's rule for its cost.  field == NULL: no environment test (grid is not read).
 * Nodes 0 and 1 are nodes like the others: status 2 is mpx_franka_roadmap's rule read with this validity test.
 * The field is an APPROXIMATION.  Distance is 1-Lipschitz, so the trilinear interpolant of exact nodal distances is within
 * (sqrt(3)/2) h of the true distance: a row may get status 2 or 1 where the exact swept-sphere test would not, and a path
 * found here may graze the cloud.  The roadmap therefore only SEEDS: mpx_franka_plan_cloud_seeded judges what it returns
 * by the exact test, and a row without a seed is simply planned without one.  field_slack >= 0 [m] widens the threshold:
 * 0 uses the field as it is (unbiased: it steers, as in the planner); 0.866 h makes the roadmap conservative.
 * Refused before any launch: what mpx_franka_roadmap refuses (T, the options, S > 64, env_offset), a bad grid (with a
 * field), point_radius or field_slack negative or not finite, a field with S == 0, and a field whose
 *   trunc <= MPX_FRANKA_MAX_SPHERE_RADIUS + point_radius + max(clearance, 0) + (check_margin + field_slack)
 * (an obstacle between trunc and the threshold would be missed silently).  The largest radius is NOT read from sph_radii
 * (device memory): it is bounded by MPX_FRANKA_MAX_SPHERE_RADIUS, the largest radius of the library's own sphere table
 * (the base link's); a caller with larger spheres leaves that room in trunc itself.
 * No allocation, no scratch, no global atomics; one kernel on `stream` (capturable).  B == 0 launches nothing.         */
#define MPX_FRANKA_MAX_SPHERE_RADIUS 0.08f
int mpx_franka_roadmap_cloud(const float *q_start, const float *q_goal, int B, int T, float finger, const float *limits,
                             const float *sph_centers, const float *sph_radii, const int32_t *sph_link, int S,
                             const float *field, const mpx_field_grid *grid, float point_radius, float field_slack,
                             const mpx_roadmap_options *options, uint64_t seed, int64_t env_offset, float *traj,
                             int32_t *status, int32_t *path, int32_t *hops, float *nodes, uint8_t *edge_state,
                             int32_t *rounds, mpx_stream_t stream);

/* Shortcutting of a joint-space polyline per problem, between a roadmap and the seeded optimiser: where the reference's
 * data generator asks its planner for shortcut = True (data_pipeline/gen_data.py:131-143).  A STAND-IN, valid by this
 * engine's sphere model; no parity with OMPL's path simplifier is claimed.  One workgroup per problem, no randomness (no
 * seed, no env_offset): row b depends on row b's inputs alone.
 *   points float32 [B,Pin,7], count int32 [B]: the polyline of problem b is its first count_b rows, 2 <= Pin <=
 *   MPX_ROADMAP_MAX_NODES.  The caller vouches for it: its own segments are never tested.  (There is no limits operand:
 *   a chord between two vertices inside a box of joint limits lies inside it.)
 *   status int32 [B]: 0 a polyline is returned, shortened or unchanged; 2 a bad row -- count < 2, count > Pin or a vertex
 *   that is not finite -- for which no chord is tested.  There is no status 1: the input is always a fallback.
 *   A configuration is VALID by mpx_franka_roadmap's clause (mpx_franka_shortcut) or by mpx_franka_roadmap_cloud's
 *   (mpx_franka_shortcut_cloud: point_radius, field_slack, "outside the grid or saturated: free", field == NULL: no
 *   environment test), with this struct's check_margin, clearance and check_self.
 *   Length of a segment (a,b): mpx_franka_roadmap's w.  CHORD from a to e, a before e in the pass's order: d = q_e - q_a,
 *   n = min(2^20, max(1, (int)ceilf(w / resolution))) pieces, interior configuration i = 1 .. n-1 is
 *   fma((float)i / (float)n, d, q_a); the chord is BLOCKED exactly when an interior configuration is invalid (the
 *   roadmap's edge test, from the end that comes first).
 *   Pass p = 0 .. passes-1, skipped once the polyline has two vertices.  An odd pass reverses the polyline's vertices,
 *   does the steps below and reverses the result back.
 *   Densify.  With v_0 .. v_h the pass's vertices, w_i = |v_{i+1} - v_i|, L = w_0 + .. + w_{h-1} summed in that order in
 *   float32 and extra = P - (h+1), P = options->points: edge i, i ascending, gets m_i = min((int)floorf(w_i * (float)extra
 *   / L), what is left of extra) interior points (the product first); every m_i is 0 when extra <= 0 or L is 0 or not
 *   finite.  Interior point k = 1 .. m_i is fma((float)k / (float)(m_i+1), v_{i+1} - v_i, v_i); the vertices are copied.
 *   The dense polyline d_0 .. d_{N-1} has N = h + 1 + sum m_i <= P points.
 *   Greedy.  Anchor a = 0, d_0 is kept; until a = N-1: lo = a+1, hi = N-1 (the segment a -> lo is part of the pass's
 *   polyline and taken as free).  While hi > lo one LEVEL tests the chords from a to the probes lo + (span k + K-1) / K
 *   (integer division), k = 1 .. K, span = hi - lo, K = options->fanout, equal probes merged; a level's chords are laid out
 *   probe ascending, `chords` counts them and `configs` their interior configurations.  If the chord to hi is free, lo =
 *   hi and the search ends.  Otherwise lo becomes the largest probe below hi whose chord is free (kept if none is), and hi
 *   becomes (the smallest probe above the new lo) - 1.  Then d_lo is kept and a = lo.  K = 1 is the linear scan from the
 *   far end; K >= span tests every point of the span at once.
 *   Every edge of the returned polyline is therefore a chord tested free here, or a piece of an edge of the polyline its
 *   pass started from (in exact arithmetic: a dense point is on its edge to float32 rounding).
 *   points_out [B,P,7], count_out int32 [B]: the returned polyline, NaN rows behind it (status 2: count_out 0, all NaN).
 *   Its first and last vertex are bit-equal to the input's.  length float32 [B,2]: the input's and the returned
 *   polyline's length, each summed in path order in float32 (NaN with status 2).  Optional: chords int32 [B], configs
 *   int32 [B] (0 with status 2).
 *   traj [B,T,7]: mpx_franka_roadmap's clause "traj" over the returned polyline, by the same statements (one edge: the
 *   planner's line bit for bit; else resampled and rounded by smooth_passes passes).  With passes = 0 and the vertices
 *   nodes[path] of a roadmap it is that roadmap's traj bit for bit.  Rows with status 2 are NaN.
 *   T, finger, the sphere table, the primitives, field, grid, point_radius and field_slack exactly as for
 *   mpx_franka_roadmap / mpx_franka_roadmap_cloud.
 * Refused before any launch: what those entries refuse about T, S, M1, M2, the field and NULL pointers; Pin outside 2 ..
 * MPX_ROADMAP_MAX_NODES; points outside Pin .. MPX_ROADMAP_MAX_NODES; passes < 0; fanout outside 1 ..
 * MPX_SHORTCUT_MAX_FANOUT; resolution <= 0 or NaN; smooth_passes < 0; check_margin < 0; a NaN clearance.
 * One workgroup of 256 threads per problem, everything but the field in LDS (35 352 B at 256 points, 27 160 B for the
 * cloud form).  No allocation, no scratch, no global atomics; one kernel on `stream` (capturable).  B == 0 launches nothing. */
#define MPX_SHORTCUT_DEFAULT_POINTS 64
#define MPX_SHORTCUT_DEFAULT_PASSES 2
#define MPX_SHORTCUT_DEFAULT_FANOUT 4
#define MPX_SHORTCUT_MAX_FANOUT 256
typedef struct mpx_shortcut_options { /* NULL options: the defaults above, resolution MPX_ROADMAP_DEFAULT_RESOLUTION,
                                         smooth_passes MPX_ROADMAP_DEFAULT_SMOOTH_PASSES, check_margin
                                         MPX_PLAN_DEFAULT_CHECK_MARGIN, clearance 0, check_self 1 */
  int points;                         /* P: Pin .. MPX_ROADMAP_MAX_NODES, the dense polyline's points        */
  int passes;                         /* >= 0: forward, backward, forward, ...                              */
  int fanout;                         /* K: 1 .. MPX_SHORTCUT_MAX_FANOUT probes per level                   */
  float resolution;                   /* > 0 [rad]: the longest piece of a chord (joint-space 2-norm)       */
  int smooth_passes;                  /* >= 0: (1/4, 1/2, 1/4) passes over the resampled polyline           */
  float check_margin;                 /* >= 0 [m], as in mpx_plan_options                                   */
  float clearance;                    /* [m], added to the radii                                            */
  int check_self;                     /* non-zero: self collisions invalidate a configuration               */
} mpx_shortcut_options;
int mpx_franka_shortcut(const float *points, const int32_t *count, int B, int Pin, int T, float finger,
                        const float *sph_centers, const float *sph_radii, const int32_t *sph_link, int S,
                        const float *cub_inv_frames, const float *cub_dims, int M1, const float *cyl_inv_frames,
                        const float *cyl_radii, const float *cyl_heights, int M2, const mpx_shortcut_options *options,
                        float *traj, int32_t *status, float *points_out, int32_t *count_out, float *length, int32_t *chords,
                        int32_t *configs, mpx_stream_t stream);
int mpx_franka_shortcut_cloud(const float *points, const int32_t *count, int B, int Pin, int T, float finger,
                              const float *sph_centers, const float *sph_radii, const int32_t *sph_link, int S,
                              const float *field, const mpx_field_grid *grid, float point_radius, float field_slack,
                              const mpx_shortcut_options *options, float *traj, int32_t *status, float *points_out,
                              int32_t *count_out, float *length, int32_t *chords, int32_t *configs, mpx_stream_t stream);

/* mpx_gripper_roadmap against a POINT CLOUD, read through its distance field: the guide of mpx_franka_follow_cloud where
 * there are no primitives to plan the gripper through.  Still the STAND-IN for the reference's OMPL end-effector planner,
 * NOT a port of it.  Every clause of mpx_gripper_roadmap's contract holds unchanged -- the gripper's rows of the sphere
 * table (links 9 / 12 / 13) and where a pose puts them, the self test on the three frame origins, the nodes (Philox stream
 * 17 keyed by (seed, GLOBAL problem id, node): the same seed gives the same nodes as mpx_gripper_roadmap, bit for bit), the
 * metric, the pieces and the nlerp of an edge, the search, the statuses, path / hops / nodes / edge_state / rounds, the
 * resampling to W guide poses with rows 0-2 of the last one goal_pose's bit for bit, NaN rows where status != 0, the
 * options with the same defaults -- except the ENVIRONMENT half of what makes a pose invalid:
 *   some gripper sphere s is BLOCKED.  Its centre c is placed from the pose as stated there, in float32; (inside, D) =
 *   mpx_cloud_field_sample's INSIDE and dist of `field` [B,nz,ny,nx] (environment b of THIS call, built by
 *   mpx_cloud_field_build on `grid`) at c.  Blocked: c is inside the grid AND D < trunc AND
 *       d <= check_margin + field_slack,   d = ((D - point_radius) - r_s) - clearance
 *   (mpx_franka_roadmap_cloud's rule, in the same words: d in that order in float32, the right-hand side summed once on
 *   the host in float32).  A centre outside the grid, or where the field is saturated, counts as FREE; a NaN centre is
 *   outside the grid and reads no memory.  field == NULL: no environment test (grid is not read); S may then be 0 and the
 *   self test still runs.
 * The field is an APPROXIMATION, within (sqrt(3)/2) h of the true distance (see mpx_franka_roadmap_cloud): a row may get
 * status 2 or 1 where the exact swept-sphere test would not object, and a guide pose may graze the cloud.  Nothing here is
 * an exact verdict: the poses only GUIDE mpx_franka_follow_cloud, which judges its trajectory by the exact test.
 * field_slack >= 0 [m] widens the threshold: 0 uses the field as it is, 0.866 h makes the roadmap conservative.
 * Refused before any launch: what mpx_gripper_roadmap refuses (the options, W, S > 64, env_offset, B x W x 16 >= 2^31, NULL
 * outputs or operands) and what mpx_franka_roadmap_cloud refuses about the field: a bad grid (with a field), point_radius or
 * field_slack negative or not finite, a field with S == 0, and a field whose
 *   trunc <= MPX_FRANKA_MAX_SPHERE_RADIUS + point_radius + max(clearance, 0) + (check_margin + field_slack)
 * -- the joint roadmap's bound although the gripper's largest sphere is smaller: one rule for every reader of a field.
 * One workgroup of 256 threads per problem, LDS 8192 B below mpx_gripper_roadmap's (no primitive rows: 33 804 B at 256
 * nodes), the field read from global memory.  No allocation, no scratch, no global atomics; one kernel on `stream`
 * (capturable).  B == 0 launches nothing (a bad option is still refused).                                              */
int mpx_gripper_roadmap_cloud(const float *start_pose, const float *goal_pose, int B, int W, const float *bounds, float finger,
                              const float *sph_centers, const float *sph_radii, const int32_t *sph_link, int S,
                              const float *field, const mpx_field_grid *grid, float point_radius, float field_slack,
                              const mpx_gripper_roadmap_options *options, uint64_t seed, int64_t env_offset, float *poses,
                              int32_t *status, int32_t *path, int32_t *hops, float *nodes, uint8_t *edge_state,
                              int32_t *rounds, mpx_stream_t stream);

/* Shortcutting of an SE(3) polyline of the free-flying gripper per problem, between a gripper roadmap and the follower:
 * mpx_franka_shortcut's algorithm over mpx_gripper_roadmap's metric, edge pose and validity.  Part of the same STAND-IN for
 * the reference's end-effector planner (data_pipeline/gen_data.py:156-189, an asymptotically optimal planner), NOT a port of
 * it; valid by this engine's sphere model.  One workgroup per problem, no randomness (no seed, no env_offset): row b depends
 * on row b's inputs alone.
 *   points float32 [B,Pin,7], count int32 [B]: the polyline of problem b is its first count_b rows, 2 <= Pin <=
 *   MPX_ROADMAP_MAX_NODES; a vertex is (p, q), position and unit quaternion (x, y, z, w), a node of mpx_gripper_roadmap.
 *   The caller vouches for its segments: they are never tested.  The sign of an input quaternion is free (q and -q give the
 *   same lengths, the same interior rotations and the same verdicts).
 *   status int32 [B]: 0 a polyline is returned, shortened or unchanged; 2 a bad row -- count < 2, count > Pin, a vertex that is
 *   not finite, or a vertex quaternion whose |q|^2 = fma(q_3, q_3, fma(q_2, q_2, fma(q_1, q_1, q_0 q_0))) is not within
 *   2^-10 of 1 (|(|q|^2) - 1| <= 2^-10 passes: a quaternion far from unit length would make NaN poses, which every
 *   comparison calls free) -- for which nothing is tested.  There is no status 1, as for mpx_franka_shortcut.
 *   Geometry.  The length of a segment (a,b) is mpx_gripper_roadmap's w with this struct's rot_weight, (2 rot_weight)^2
 *   rounded as there; a CHORD from a to e, a before e in the pass's order, has that contract's n pieces of w(a,e) at this
 *   struct's resolution and the interior poses i = 1 .. n-1 of its edge (a,e): f = (float)i / (float)n, p by fma, q by nlerp
 *   toward sigma_ae q_e, taken from a, the end that comes first.  The chord is BLOCKED exactly when an interior pose is
 *   invalid.
 *   A pose is VALID by mpx_gripper_roadmap's clause (mpx_gripper_shortcut: the gripper's rows of the sphere table, links 9 /
 *   12 / 13, against the live primitives; the self test on the three frame origins) or by mpx_gripper_roadmap_cloud's
 *   (mpx_gripper_shortcut_cloud: the 8-load field sample, point_radius, field_slack, "outside the grid or saturated: free",
 *   field == NULL: no environment test and S may be 0), with this struct's check_margin, clearance and check_self.
 *   Pass, Densify, Greedy: mpx_franka_shortcut's clauses, word for word, with "w_i" the length above and an interior point
 *   k = 1 .. m_i of densify the edge pose of (v_i, v_{i+1}) at f = (float)k / (float)(m_i+1) (fma positions, nlerp), the
 *   probes lo + (span k + K-1) / K, `chords` and `configs` (interior POSES here) counted as there.  An odd pass reverses the
 *   vertices, does the steps and reverses the result back; an nlerp taken from the other end may return -q where the even
 *   pass returns q: the same rotation.
 *   points_out [B,P,7], count_out int32 [B]: the returned polyline, NaN rows behind it (status 2: count_out 0, all NaN).  Its
 *   first and last vertex are bit-equal to the input's.  length float32 [B,2]: the input's and the returned polyline's
 *   length, each summed in path order in float32 (NaN with status 2).  Optional: chords int32 [B], configs int32 [B] (0 with
 *   status 2).  (w takes the CHORD of a quaternion pair and an nlerp runs along the arc, so the pieces of an edge sum to
 *   slightly more than the edge: a polyline from which nothing is cut may come back a few parts in a million longer.)
 *   poses [B,W,4,4], 1 <= W <= MPX_FOLLOW_MAX_POSES: mpx_gripper_roadmap's clause "poses" over the returned polyline, by the
 *   same statements (c_i, s_t, the last edge with c_i <= s_t, the edge's nlerp in polyline order).  goal_pose [B,4,4] or
 *   NULL: rows 0-2 of pose W-1 are goal_pose's bit for bit; with NULL they are [R | p] of the last vertex itself.  Row 3 of
 *   every pose is (0, 0, 0, 1).  Rows with status 2 are NaN (all 16 entries).  With passes = 0, the vertices nodes[path] of a
 *   gripper roadmap and that roadmap's goal_pose, poses is that roadmap's poses bit for bit.
 *   finger, the sphere table, the primitives, field, grid, point_radius and field_slack exactly as for mpx_gripper_roadmap /
 *   mpx_gripper_roadmap_cloud.
 * Refused before any launch: what mpx_franka_shortcut refuses about Pin, points, passes, fanout, resolution, check_margin,
 * clearance and NULL pointers; what mpx_gripper_roadmap refuses about W, S > 64, M1 / M2 and rot_weight; B x W x 16 or
 * B x P x 7 >= 2^31; for the cloud form what mpx_gripper_roadmap_cloud refuses about the field, the grid, point_radius,
 * field_slack and trunc.  B == 0 launches nothing (a bad option is still refused).
 * One workgroup of 256 threads per problem, everything but the field in LDS: the 128 primitive rows (8192 B), the 64 gripper
 * sphere rows and their count (1028 B) and the shortcut's arrays without a trajectory buffer (92 P + 24 B): 32 796 B at 256
 * points, 24 604 B for the cloud form (no primitive rows).  No allocation, no scratch, no global atomics; one kernel on
 * `stream` (capturable).                                                                                                */
typedef struct mpx_gripper_shortcut_options { /* NULL options: MPX_SHORTCUT_DEFAULT_POINTS / _PASSES / _FANOUT, resolution
                                                 MPX_GRIPPER_ROADMAP_DEFAULT_RESOLUTION, rot_weight
                                                 MPX_GRIPPER_ROADMAP_DEFAULT_ROT_WEIGHT, check_margin
                                                 MPX_PLAN_DEFAULT_CHECK_MARGIN, clearance 0, check_self 1 */
  int points;                                 /* P: Pin .. MPX_ROADMAP_MAX_NODES, the dense polyline's points   */
  int passes;                                 /* >= 0: forward, backward, forward, ...                         */
  int fanout;                                 /* K: 1 .. MPX_SHORTCUT_MAX_FANOUT probes per level              */
  float resolution;                           /* > 0 [m]: the longest piece of a chord (the metric w)          */
  float rot_weight;                           /* > 0 [m/rad]: what a radian of rotation counts in w            */
  float check_margin;                         /* >= 0 [m], as in mpx_plan_options                              */
  float clearance;                            /* [m], added to the radii                                       */
  int check_self;                             /* non-zero: the body column invalidates a pose                  */
} mpx_gripper_shortcut_options;
int mpx_gripper_shortcut(const float *points, const int32_t *count, int B, int Pin, int W, const float *goal_pose, float finger,
                         const float *sph_centers, const float *sph_radii, const int32_t *sph_link, int S,
                         const float *cub_inv_frames, const float *cub_dims, int M1, const float *cyl_inv_frames,
                         const float *cyl_radii, const float *cyl_heights, int M2,
                         const mpx_gripper_shortcut_options *options, float *poses, int32_t *status, float *points_out,
                         int32_t *count_out, float *length, int32_t *chords, int32_t *configs, mpx_stream_t stream);
int mpx_gripper_shortcut_cloud(const float *points, const int32_t *count, int B, int Pin, int W, const float *goal_pose,
                               float finger, const float *sph_centers, const float *sph_radii, const int32_t *sph_link, int S,
                               const float *field, const mpx_field_grid *grid, float point_radius, float field_slack,
                               const mpx_gripper_shortcut_options *options, float *poses, int32_t *status, float *points_out,
                               int32_t *count_out, float *length, int32_t *chords, int32_t *configs, mpx_stream_t stream);

/* mpx_franka_follow against a POINT CLOUD: the same follower -- still the STAND-IN for the reference's Geometric Fabrics
 * expert, NOT Lula's fabric, no parity claimed.  Every clause of mpx_franka_follow's contract holds unchanged -- the state,
 * the switch and the stop, the attractor, the barrier, the damping, the clamp, the dense path and arc, the retiming, the
 * jerk, self and miss bits, status 0 / 1 / 2, NaN rows, continuing a rollout from q_end / v_end / progress_end, one wave per
 * problem, lane = collision sphere, the fixed-order reduction, no randomness -- with two substitutions:
 *   Obstacle term of one step (clause 5).  (inside, D, n) = mpx_cloud_field_sample's INSIDE, dist and grad of `field`
 *   [B,nz,ny,nx] (environment b of THIS call, built by mpx_cloud_field_build on `grid`) at the sphere centre x_s;
 *   d_s = ((D - point_radius) - r_s) - clearance (mpx_franka_plan_cloud's expression, in that order, in float32); the sphere
 *   is active only where D < trunc and d_s < epsilon: c'(d) = -1 for d < 0, else (d - epsilon) / epsilon; its term is
 *   c'(d_s) n (n as sampled, not normalised) through the joints upstream of its link, as in mpx_franka_plan_cloud.  A centre
 *   outside the grid or in the saturated band contributes nothing.  field == NULL: no obstacle term (grid is not read).
 *   Environment verdict (bit 0 of bits).  A row carries it exactly when mpx_franka_cloud_collision flags its refined
 *   configurations [B,R,7], R = (T-1) substeps + 1 (r = t substeps + i, mpx_franka_plan's fma), against environment b's
 *   cloud (cloud, strides, N, counts: as there) with this point_radius and clearance = options->clearance +
 *   options->check_margin summed in float32: that entry itself is called, flags only.  The field steers and never judges.
 *   cloud == NULL, N == 0, S == 0 or counts[b] == 0: no environment test for that row.
 *   status 2: mpx_franka_follow's rule, the configuration test of a FRESH rollout's q_start (progress_init == NULL) being
 *   that call on q_start as [B,1,7] and, with check_self, the planner's self test; with progress_init given neither is made.
 * Hence: with field == NULL and no cloud every output is bit-equal to mpx_franka_follow's without primitives.
 * scratch: device memory, 16-byte aligned, at least mpx_franka_follow_cloud_scratch(B, T, substeps) bytes (-1 for sizes the
 * entry refuses), owned by the caller, free when the stream has passed the call.  No allocation, no host synchronisation;
 * every step is enqueued on `stream` (a memset of the flags, for a fresh rollout the flags call on q_start, the rollout
 * kernel, the flags call on the refined configurations, a finish kernel that writes status, bits, traj and traj_any).
 * Refused before any launch: what mpx_franka_follow refuses (W, T, the options, S > 64, NULL outputs or operands), a bad
 * grid (with a field), point_radius negative, a cloud with N > 0 and a point stride below 3, a field or a cloud with S == 0,
 * a scratch that is too small, NULL or not 16-byte aligned.  B == 0 launches nothing.                                   */
int64_t mpx_franka_follow_cloud_scratch(int B, int T, int substeps);
int mpx_franka_follow_cloud(const float *q_start, const float *poses, int B, int W, int T, float finger, const float *limits,
                            const float *sph_centers, const float *sph_radii, const int32_t *sph_link, int S,
                            const float *field, const mpx_field_grid *grid, const float *cloud, int64_t cloud_batch_stride,
                            int cloud_point_stride, int N, const int32_t *counts, float point_radius, const float *v_init,
                            const int32_t *progress_init, const mpx_follow_options *options, float *path, float *arc,
                            int32_t *status, int32_t *bits, int32_t *steps, float *traj, float *traj_any, float *q_end,
                            float *v_end, int32_t *progress_end, void *scratch, int64_t scratch_bytes, mpx_stream_t stream);

/* ---- split-bf16 ("bf16x3") dense layers: the opt-in fast mode of mpx_linear / mpx_linear_rowmax ------
 * Every fp32 product is evaluated as x_hi*w_hi + x_hi*w_lo + x_lo*w_hi on the bf16 matrix cores (fp32
 * accumulate).  Split operands are held in the PAIRS form: a row holds, per group of 16 k-values,
 * [hi x 16 | lo x 16] bf16 (hi = bf16(v), lo = bf16(v - hi)), K padded with zeros to Kp = roundup(K, 16):
 * [rows, ld >= 2 Kp] bf16 -- the same bytes as the fp32 rows.  mpx_split_bf16 converts fp32 rows [R, K]
 * (weights [N, K], once; or activations) into pairs.  Same argument meaning as the fp32 entry points otherwise;
 * weights are always passed as pairs with ld = 2 Kp.
 *   mpx_linear_bf16x3 / mpx_linear_rowmax_bf16x3: fp32 activations (split while staged), fp32 result.
 *   mpx_linear_bf16x3_to_pairs: the same, result written as pairs (N and ldp multiples of 4, ldp >= 2 Np).
 *   mpx_linear_bf16x3_pairs: activations already in pairs (a_pairs [M, lda], K a multiple of 16, lda of 8; under
 *     4 GB), result EITHER fp32 rows (y) OR pairs (y_pairs); the other pointer NULL.
 *   mpx_linear_rowmax_bf16x3_pairs: ReLU + max over each group of rows = 128 rows, as fp32 (y) or pairs (y_pairs).
 * Chains of layers (the group-all module's 259 -> 512 -> 512 -> 1024 MLP, model.py:383) keep their activations in
 * pairs: a value is split once, by the epilogue that produces it, and every form accumulates in the same order, so a
 * chain through pairs equals the chain through fp32 rows bit for bit.                                            */
int mpx_split_bf16(const float *x, int ldx, int64_t R, int K, void *pairs, int ldp, mpx_stream_t stream);
int mpx_linear_bf16x3(const float *x, int ldx, const void *w_pairs, const float *bias, int M, int N, int K,
                      int act, float *y, int ldy, mpx_stream_t stream);
int mpx_linear_rowmax_bf16x3(const float *x, int ldx, const void *w_pairs, const float *bias, int M, int N,
                             int K, int rows, float *y, int ldy, mpx_stream_t stream);
int mpx_linear_bf16x3_to_pairs(const float *x, int ldx, const void *w_pairs, const float *bias, int M, int N,
                               int K, int act, void *y_pairs, int ldp, mpx_stream_t stream);
int mpx_linear_bf16x3_pairs(const void *a_pairs, int lda, const void *w_pairs, const float *bias, int M, int N,
                            int K, int act, float *y, int ldy, void *y_pairs, int ldp, mpx_stream_t stream);
int mpx_linear_rowmax_bf16x3_pairs(const void *a_pairs, int lda, const void *w_pairs, const float *bias, int M,
                                   int N, int K, int rows, float *y, int ldy, void *y_pairs, int ldp,
                                   mpx_stream_t stream);

/* The group-all module's first two layers (272 -> 512 -> 512, ReLU each; model.py:377-383) in bf16x3 as ONE kernel: a
 * workgroup per environment, the rows divided among its waves, activations in registers from layer to layer, the weights
 * streamed through an LDS ring once per environment (csrc/sa3_front_bf16.hip).  x: fp32 rows [B * 128, ldx >= 272]
 * ([xyz | f | 0], 16-byte aligned); y_pairs: [B * 128, ldp >= 1024] bf16 in the pairs form with the k-steps in the KERNEL's
 * channel order -- the operand of mpx_linear_rowmax_bf16x3_pairs with the weight pairs of mpx_sa3_front_bf16x3_w3_pairs
 * (the same columns permuted).  Equal to mpx_linear_bf16x3_to_pairs + mpx_linear_bf16x3_pairs to rounding (the 16 products
 * of a k-step enter the MFMA in another order, the bias is added first), not bit for bit.
 * pack: mpx_sa3_front_bf16x3_pack_size bytes (host call; -1: unsupported widths), written by mpx_sa3_front_bf16x3_pack from
 * the fp32 weights w1 [c1, k1_real <= K1], w2 [c2, c1] and biases.                                                    */
int64_t mpx_sa3_front_bf16x3_pack_size(int K1, int c1, int c2);
int mpx_sa3_front_bf16x3_pack(const float *w1, int k1_real, const float *b1, const float *w2, const float *b2, int K1,
                              int c1, int c2, void *pack, mpx_stream_t stream);
int mpx_sa3_front_bf16x3_w3_pairs(const float *w3, int c3, int c2, void *w3_pairs, mpx_stream_t stream);
int mpx_sa3_front_bf16x3(const float *x, int ldx, int B, int rows, const void *pack, void *y_pairs, int ldp,
                         mpx_stream_t stream);

/* ---- training losses with analytic gradients (row N1; mpinets/loss.py:31-166) -------------------- */

/* collision_loss (loss.py:48-95) on points [B,N,3] (strides in floats): per environment
 * loss_sum[b] = sum_n max(0, margin - min(cuboid sdf, cylinder sdf)); the reference's mean is
 * sum_b loss_sum[b] / (B*N).  grad_points (optional, strided like points) receives
 * d(loss_sum[b]) / d(point): the autograd of geometry.py:256-288 / :478-507 restated analytically.
 * A point with a NaN or infinite coordinate takes no part: it adds nothing to loss_sum[b] and its
 * gradient row is +0 (the reference returns NaN there); the other rows are as without it.
 * frames / dims / radii / heights as for mpx_cuboid_sdf / mpx_cylinder_sdf.                          */
int mpx_collision_hinge(const float *points, int64_t batch_stride, int point_stride, int B, int N,
                        const float *cub_frames, const float *cub_dims, int M1, const float *cyl_frames,
                        const float *cyl_radii, const float *cyl_heights, int M2, float margin,
                        float *loss_sum, float *grad_points, int64_t grad_batch_stride,
                        int grad_point_stride, mpx_stream_t stream);

/* point_match_loss (loss.py:31-45) on contiguous input/target [B, n_per_env]: sums[b] =
 * {sum d^2, sum |d|}; grad_input (optional) = w_sq*2*d + w_abs*sign(d) -- pass w = 1/(B*n_per_env)
 * for the reference's two mean reductions.                                                           */
int mpx_point_match(const float *input, const float *target, int B, int n_per_env, float w_sq, float w_abs,
                    float *sums, float *grad_input, mpx_stream_t stream);

/* Backward of mpx_franka_cloud (robofin FrankaSampler.sample under autograd; loss.py:142-147):
 * grad_q[b,k] = sum_points grad_points[b,p] . d(point)/d(q_k), joint angles in radians.             */
int mpx_franka_cloud_grad(const float *q, int B, float finger, const float *table_pts,
                          const int32_t *table_link, const int32_t *subset, int n, const float *grad_points,
                          int64_t grad_batch_stride, int grad_point_stride, float *grad_q,
                          mpx_stream_t stream);

/* ---- backward of the dense layers (row N1): y = act(x . W^T + b) ------------------------------------
 * dX is the forward kernel on the transposed weights: mpx_linear(dZ, W^T).  mpx_act_backward forms
 * dZ = dY * act'(y) from the layer OUTPUT y (contiguous, n elements).  mpx_linear_wgrad computes
 * dW [N,K] = dZ^T . x and db [N] = column sums of dZ (optional) with the reduction over the M rows split across
 * workgroups; the splits' partial tiles go through `scratch` (mpx_linear_wgrad_scratch(M,N,K) floats) and are
 * added in a fixed order (deterministic).  N, K, ldx, lddy multiples of 4.                                  */
int mpx_act_backward(const float *dy, const float *y, int64_t n, int act, float *dz, mpx_stream_t stream);
/* dX with the previous layer's elementwise backward in the GEMM epilogue: y [M,N] = (x [M,K] . w [N,K]^T) * act'(dact_of)
 * (dact_of [M,N] = that layer's OUTPUT rows, leading dimension lddact; dact = its activation; MPX_ACT_NONE: plain
 * product).  Same arithmetic as mpx_linear(x, w) followed by mpx_act_backward.  loss.py / model.py:185-240 via autograd. */
int mpx_linear_dact(const float *x, int ldx, const float *w, int M, int N, int K, const float *dact_of,
                    int lddact, int dact, float *y, int ldy, mpx_stream_t stream);
/* The training GEMMs in the split-bf16 arithmetic of the `bf16x3` mode (three bf16 MFMAs per fp32 product, fp32
 * accumulate, fp32 master weights: the engine's form of the reference's precision=16, run_training.py:112): the forward is
 * mpx_linear_bf16x3; dX = mpx_linear_bf16x3_dact (w_pairs = mpx_split_bf16 of the TRANSPOSED weights); dW / db =
 * mpx_linear_wgrad_bf16x3 (same arguments, scratch and split reduction as mpx_linear_wgrad).                           */
int mpx_linear_bf16x3_dact(const float *x, int ldx, const void *w_pairs, int M, int N, int K, const float *dact_of,
                           int lddact, int dact, float *y, int ldy, mpx_stream_t stream);
int mpx_linear_wgrad_bf16x3(const float *dy, int lddy, const float *x, int ldx, int M, int N, int K, float *dw,
                            float *db, float *scratch, mpx_stream_t stream);
int64_t mpx_linear_wgrad_scratch(int M, int N, int K);
int mpx_linear_wgrad(const float *dy, int lddy, const float *x, int ldx, int M, int N, int K, float *dw,
                     float *db, float *scratch, mpx_stream_t stream);

/* backward of mpx_groupnorm_leaky on [M, C]: dx, dgamma [C], dbeta [C]; stats = scratch of 2*M*groups floats    */
int mpx_groupnorm_leaky_grad(const float *x, const float *gamma, const float *beta, const float *dy, int M,
                             int C, int groups, float eps, float *dx, float *dgamma, float *dbeta,
                             float *stats, mpx_stream_t stream);

/* ---- differentiable grouping + max-pool of the set-abstraction stack (row N1) --------------------
 * The reference trains through pointnet2_ops' QueryAndGroup / max-pool (model.py:366-383).  Here a
 * neighbourhood contributes only its distinct neighbours (cnt from mpx_ball_query; padding repeats
 * the first hit and neither a max nor its gradient sees repeats): rows of one [R, 3+C] matrix,
 * query q owning rows offsets[q] .. offsets[q+1] (offsets int64 [B*npoint+1] = exclusive prefix
 * sum of max(cnt,1)).                                                                              */

/* rows[offsets[q]+r] = [xyz[idx[q,r]] - new_xyz[q] | feat[idx[q,r]]]  (QueryAndGroup, use_xyz=True) */
int mpx_pack_rows(const float *xyz, int xyz_stride, const float *new_xyz, int new_stride,
                  const float *feat, int feat_stride, int C, const int32_t *idx, const int32_t *cnt,
                  const int64_t *offsets, int B, int N, int npoint, int nsample, float *rows,
                  mpx_stream_t stream);
/* ... with the rows `ld` >= 3 + C floats apart and the columns behind 3 + C zero-filled (ld % 4 == 0: no padding copy in
 * front of the GEMMs)                                                                                 */
int mpx_pack_rows_ld(const float *xyz, int xyz_stride, const float *new_xyz, int new_stride, const float *feat,
                     int feat_stride, int C, const int32_t *idx, const int32_t *cnt, const int64_t *offsets, int B, int N,
                     int npoint, int nsample, float *rows, int ld, mpx_stream_t stream);
/* backward: grad_feat[b, idx[q,r], c] += grad_rows[offsets[q]+r, 3+c] (atomic adds; grad_feat pre-zeroed) */
int mpx_pack_rows_grad(const float *grad_rows, int C, const int32_t *idx, const int32_t *cnt,
                       const int64_t *offsets, int B, int N, int npoint, int nsample, float *grad_feat,
                       int feat_stride, mpx_stream_t stream);
int mpx_pack_rows_grad_ld(const float *grad_rows, int ld, int C, const int32_t *idx, const int32_t *cnt,
                          const int64_t *offsets, int B, int N, int npoint, int nsample, float *grad_feat, int feat_stride,
                          mpx_stream_t stream); /* (gradient rows ld >= 3 + C floats apart) */
/* out[q,c] = max over the rows of segment q of y[R,C]; arg[q,c] = first row attaining it           */
int mpx_segment_max(const float *y, int C, const int64_t *offsets, int64_t Q, float *out, int out_stride,
                    int64_t *arg, mpx_stream_t stream);
/* backward: grad_y[arg[q,c], c] = grad_out[q,c] (grad_y pre-zeroed)                                  */
int mpx_segment_max_grad(const float *grad_out, int grad_stride, const int64_t *arg, int64_t Q, int C,
                         float *grad_y, mpx_stream_t stream);
/* the same with the backward of the activation in front of the pool folded in: out [Q, >= C] = the pooled rows
 * (= the activation's output at the arg-max): grad_y[r, c] = (r == arg[q,c]) ? grad_out[q,c] * act'(out[q,c]) : 0 for
 * EVERY row r of segment q -- grad_y needs no zero fill                                                         */
int mpx_segment_max_grad_act(const float *grad_out, int grad_stride, const int64_t *arg, const float *out,
                             int out_stride, const int64_t *offsets, int64_t Q, int C, int act, float *grad_y,
                             mpx_stream_t stream);
/* Forward of [dense layer + activation + segment max-pool] without the [M, N] matrix in memory: pooled[q, n] = max over the
 * rows r with seg[r] == q of act(x[r] . w[n] + bias[n]), arg[q, n] = the first such row -- mpx_linear followed by
 * mpx_segment_max, bit for bit (the same tile kernel; its epilogue folds the tile into 64-bit {value, ~row} keys with
 * atomicMax).  seg int32 [M]: the segment of every row, non-decreasing, every q in [0, Q) present; keys: Q*N*8 bytes of
 * scratch (8-byte aligned); pooled [Q, >= N] (ldp floats apart), arg int64 [Q, N].  _bf16x3: the product in split bf16
 * (w_pairs from mpx_split_bf16, as mpx_linear_bf16x3).  (Reference: pointnet2_ops' SharedMLP + max_pool2d, model.py:366-383.) */
int mpx_linear_segmax(const float *x, int ldx, const float *w, const float *bias, int M, int N, int K, int act,
                      const int32_t *seg, int64_t Q, void *keys, float *pooled, int ldp, int64_t *arg, mpx_stream_t stream);
int mpx_linear_segmax_bf16x3(const float *x, int ldx, const void *w_pairs, const float *bias, int M, int N, int K, int act,
                             const int32_t *seg, int64_t Q, void *keys, float *pooled, int ldp, int64_t *arg,
                             mpx_stream_t stream);
/* Backward of [dense layer (W [C,K], b) + activation `act` + segment max-pool] that never forms the [R, C] gradient in
 * front of the pool: per (query, channel) only the arg-max row carries gz[q,c] = grad_out[q,c] * act'(out[q,c]) (out = the
 * pooled rows).  x [R, >= K] = the layer's INPUT rows (ldx floats apart), arg = mpx_segment_max's (global row numbers).
 *   mpx_pool_wgrad: dw[c,k] = sum_q gz[q,c] * x[arg[q,c], k], db[c] = sum_q gz[q,c]  (db NULL or == dw + C*K: one fixed-order
 *                   reduction over the query splits; scratch = mpx_pool_wgrad_scratch(Q, C, K) floats);
 *   mpx_pool_dgrad: gx[r,k] = below'(x[r,k]) * sum_{c: arg[q,c] == r} gz[q,c] * w[c,k] for EVERY row r of every segment (no
 *                   zero fill needed; `below` = activation code of the layer that produced x, 0 = none; max_rows: reserved,
 *                   ignored; C <= 65535).
 * fp32 FMAs in a fixed order: deterministic; the same sums as mpx_segment_max_grad_act + mpx_linear_wgrad / mpx_linear_dact
 * in another summation order.  (Reference: the autograd of pointnet2_ops' QueryAndGroup + max_pool2d, model.py:366-383.) */
int64_t mpx_pool_wgrad_scratch(int64_t Q, int C, int K);
int mpx_pool_wgrad(const float *grad_out, int grad_stride, const int64_t *arg, const float *out, int out_stride,
                   int64_t Q, int C, int act, const float *x, int ldx, int K, float *dw, float *db, float *scratch,
                   mpx_stream_t stream);
int mpx_pool_dgrad(const float *grad_out, int grad_stride, const int64_t *arg, const float *out, int out_stride,
                   const int64_t *offsets, int64_t Q, int C, int act, const float *w, int ldw, const float *x, int ldx,
                   int below, int K, int max_rows, float *gx, int ldg, mpx_stream_t stream);

/* ---- batch assembly from the dataset arrays (row N2; mpinets/data_loader.py:141-280, 390-417) ------- */

/* Per-sample joint quantities of PointCloudBase.get_inputs for a whole batch.  trajectories
 * [n_traj, L, 7] (the HDF5 `hybrid_solutions` / `global_solutions` array, resident in HBM), traj_idx
 * int64 [B] (clamped to [0, n_traj)), timestep int32 [B] (NULL = 0: the validation dataset).  Outputs: q [B,7] =
 * the waypoint (+ N(0, noise_scale) joint noise when noise_scale > 0; Philox keyed by (seed, sample_offset + row),
 * so a shard of a batch draws what the whole batch draws), clamped to the limits whenever `train` != 0
 * (data_loader.py:176-178 clamps every TRAIN sample, with or without noise), q_norm = normalize(q), sup_norm (optional) = normalize(waypoint min(t+1, L-1)),
 * target_pose [B,4,4] / target_pos [B,3] = right_gripper FK of the LAST waypoint.                  */
int mpx_batch_configs(const float *trajectories, int64_t n_traj, int L, const int64_t *traj_idx,
                      const int32_t *timestep, const float *limits, float noise_scale, uint64_t seed,
                      int64_t sample_offset, int train, int B, float finger, float *q, float *q_norm, float *sup_norm, float *target_pose,
                      float *target_pos, mpx_stream_t stream);
/* dst[b, :] = src[idx[b], :] for rows of row_floats floats (primitive rows of the sampled scenes)  */
int mpx_gather_rows(const float *src, const int64_t *idx, int B, int row_floats, float *dst,
                    mpx_stream_t stream);

/* ---- partial-view scene clouds from a depth camera (row N4; run_inference.py:194-257) ------------- */

/* Analytic ray casting of the primitives from cam_poses [B,4,4] (world-from-camera, OpenGL axes: x right,
 * y up, looking along -z, as the reference's evaluation poses are given), pinhole intrinsics in pixels,
 * image W x H.  depth [B, H*W] = distance along the pixel's ray to the nearest cuboid / cylinder, or -1 when
 * nothing is hit within far_clip or one of the robot's spheres (sph_centers [B,S,3] from mpx_franka_spheres,
 * sph_radii [S]; S = 0: no robot) is in front -- the reference removes the robot's pixels.
 * A primitive or robot sphere that CONTAINS the camera origin is invisible (the rasteriser this stands in for culls
 * back faces): only an entry into a primitive counts as a hit, never the exit through a wall or a cap.
 * Replaces PyBullet's rasteriser + depth buffer (robofin Bullet.get_pointcloud_from_camera).       */
int mpx_depth_render(const float *cam_poses, float fx, float fy, float cx, float cy, int W, int H, int B,
                     const float *cub_frames, const float *cub_dims, int M1, const float *cyl_frames,
                     const float *cyl_radii, const float *cyl_heights, int M2, const float *sph_centers,
                     const float *sph_radii, int S, float far_clip, float *depth, mpx_stream_t stream);
/* np.random.choice(len(cloud), n_out, replace=False) of run_inference.py:78-85 on the device: every valid
 * pixel gets a Philox4x32-10 key (seed, env_offset + environment, pixel); the n_out smallest keys are written as world
 * points in key order to out (strides in floats).  count [B] = valid pixels; an environment with fewer than
 * n_out of them is left untouched (the caller raises like numpy).  n_out <= 4096.  A pixel is valid when its depth
 * is >= 0 (so -0.0 is valid; -1 and NaN are not).                                                     */
int mpx_depth_select(const float *depth, const float *cam_poses, float fx, float fy, float cx, float cy,
                     int W, int H, int B, int n_out, uint64_t seed, int64_t env_offset, float *out,
                     int64_t out_batch_stride, int out_point_stride, int32_t *count, mpx_stream_t stream);

/* Cleaning of CAPTURED clouds, the step the reference's real-robot planner leaves to its caller
 * (interactive_demo/mpinets_ros/nodes/planning_node.py:78-151 asserts a [4096,3] cloud; its clean_point_cloud, :187-228,
 * crops to two boxes and draws on the host): crop, robot removal, outlier removal and the draw, for a batch.
 * Row i of environment b is the three floats at cloud + b*cloud_batch_stride + i*cloud_point_stride (strides in floats,
 * point stride >= 3, read in place as for mpx_franka_cloud_collision); the rows i < n_b exist, n_b = counts[b] clamped to
 * [0, N], or N when counts is NULL.  Every row gets a reason, the FIRST stage it fails, or 0:
 *   1  non-existent or non-finite: i >= n_b, or a coordinate is NaN or infinite
 *   2  outside the workspace (skipped when n_boxes == 0): no box j of boxes [n_boxes,6] (lo xyz, hi xyz; one set for the
 *      batch) has lo_j < p < hi_j STRICTLY on all three axes, float32 comparisons.  n_boxes <= MPX_CLEAN_MAX_BOXES
 *   3  robot (skipped when S == 0): some sphere s has d2 <= R_s*R_s with d2 = fma(dz,dz, fma(dx,dx, dy*dy)), dx = p.x - c.x
 *      (dy, dz likewise) in float32 -- the library's one squared distance -- and R_s = sph_radii[s] + robot_margin in
 *      float32.  sph_centers [B,S,3] are mpx_franka_spheres' output.  S <= MPX_CLEAN_MAX_SPHERES, robot_margin >= 0
 *   4  outlier (skipped when min_neighbors == 0): with alive1 = the rows that passed 1-3, row i is kept iff at least
 *      min_neighbors rows j != i (by index) of alive1 have d2(p_i - p_j) <= r*r, r = outlier_radius > 0, r*r in float32.
 *      A row with the same coordinates is a neighbour.  ONE pass: neighbours are counted among alive1, not among the
 *      final survivors.
 * count [B] = rows with reason 0.  reason uint8 [B,N] (optional) is written for all N rows.
 * Draw (n_out == 0: filter only; else n_out <= 4096): an environment with count[b] < n_out is left untouched in out and
 * src_index (the caller raises like numpy, as for mpx_depth_select).  Otherwise row i gets word i & 3 of
 * Philox4x32-10(counter = (i >> 2, env_offset + b, 15, 0), key = (seed lo, seed hi)) as its key, the n_out smallest
 * (key, i) pairs win and, in ascending order k, src_index[b,k] = i_k (int32 [B,n_out], optional) and out[b,k,0:3] =
 * cloud[b,i_k,0:3] bit for bit, at out + b*out_batch_stride + k*out_point_stride; nothing else of an output row is
 * touched (a slab row keeps its label column).
 * The result depends on the inputs alone: not on the grid below, nor on the order in which atomics land.
 * Stage 4 bins alive1 into a uniform grid per environment (over the bounding box of the crop boxes, else over alive1's
 * own box; cell edge >= 1.01 r, at most MPX_CLEAN_MAX_CELLS cells -- a far-away row without a crop box only makes the
 * cells coarse) and counts within the 27 cells around a row, stopping at min_neighbors.
 * scratch: device memory, 16-byte aligned, at least mpx_cloud_clean_scratch(B, N) bytes, owned by the caller and free
 * again when the call's work on the stream has finished.  Bad arguments are refused before any launch; B == 0
 * launches nothing. */
#define MPX_CLEAN_MAX_BOXES 8
#define MPX_CLEAN_MAX_SPHERES 64
#define MPX_CLEAN_MAX_CELLS 262144
int64_t mpx_cloud_clean_scratch(int B, int N);
int mpx_cloud_clean(const float *cloud, int64_t cloud_batch_stride, int cloud_point_stride, int N,
                    const int32_t *counts, int B, const float *boxes, int n_boxes, const float *sph_centers,
                    const float *sph_radii, int S, float robot_margin, float outlier_radius, int min_neighbors,
                    int n_out, uint64_t seed, int64_t env_offset, float *out, int64_t out_batch_stride,
                    int out_point_stride, int32_t *src_index, uint8_t *reason, int32_t *count, void *scratch,
                    int64_t scratch_bytes, mpx_stream_t stream);

/* ---- scene point clouds: mpinets/geometry.py:571-608 (construct_mixed_point_cloud), batched ----- */

/* For every environment: area-proportional pool sizes int(p_i*N)+500, N pool slots drawn without
 * replacement in random order (every slot gets a Philox key, the N smallest keys win in key order;
 * only the owning obstacle matters), one fresh uniform surface sample per slot, labels = shuffled
 * 1..K.  N <= 4096.  Counter RNG Philox4x32-10 keyed by
 * (seed, GLOBAL environment id = env_offset + row): results depend on nothing else, so rank r of a sharded batch
 * (env_offset = its first global environment) draws exactly what one process would for those environments.  Zero-volume primitives are skipped;
 * obstacle ids count cuboids first, then cylinders.  An environment without obstacles gets
 * ids 0xFFFF and zero points (the reference returns an empty array, geometry.py:586-587).
 *   assign uint16 [B,N] (required scratch/output), labels uint8 [B,M1+M2] (optional),
 *   n_obstacles int32 [B] (optional); out rows at out + b*out_batch_stride + j*out_point_stride
 *   receive x,y,z (and the label as float in column 3 when write_label != 0).                 */
int mpx_scene_cloud(const float *cub_centers, const float *cub_dims, const float *cub_quats, int M1,
                    const float *cyl_centers, const float *cyl_radii, const float *cyl_heights,
                    const float *cyl_quats, int M2, int B, int num_points, uint64_t seed,
                    int64_t env_offset, uint16_t *assign, uint8_t *labels, int32_t *n_obstacles, float *out,
                    int64_t out_batch_stride, int out_point_stride, int write_label,
                    mpx_stream_t stream);

/* ---- PointNet++ set abstraction: pointnet2_ops call sites model.py:27,366-383 ------------- */

/* furthest_point_sample (+ gather_operation): xyz rows at xyz + (b*N + k)*stride, first three
 * floats used.  idx int32 [B,npoint]; new_xyz (optional) rows at
 * new_xyz + (b*npoint + j)*new_stride.  Index semantics follow pointnet2_ops v3.2.0 exactly
 * (start 0, float |p|^2 <= the double 1e-3 skipped, block-size-dependent tie order).  N <= 8192.  */
int mpx_fps(const float *xyz, int B, int N, int stride, int npoint, int32_t *idx, float *new_xyz,
            int new_stride, mpx_stream_t stream);

/* Verification hook (host call, process-wide): which kernel family serves mpx_fps / mpx_ball_query.  value 1 (default) =
 * the fast kernels (one wave per small cloud / Morton-culled FPS; wave-per-query / bucketed ball query); value 0 = the
 * plain kernels they are proven against.  Indices are identical bit for bit either way; the switch lets a test run
 * both on the same clouds in one process (tests/test_gpu_soak.py).  Returns non-zero on a bad selector / value.      */
#define MPX_VARIANT_FPS 0
#define MPX_VARIANT_BALL_QUERY 1
/* 1 (default): a stream's persistent grouped-MLP launches take a private set of unit-queue counters (256 distinct
 * (device, stream) handles per process).  0: handles not seen before get none, as if all 256 were taken -- the fp32
 * launchers then run one unit per wave without a queue (same results), mpx_sa_mlp_bf16x3_factored fails with a message. */
#define MPX_VARIANT_UNIT_QUEUE 2
/* 1 (default): the flags-only form of mpx_franka_cloud_collision discards points outside the box of its workgroup's
 * spheres and stops at an environment's first hit.  0: it visits every point.  Same flags bit for bit either way.  */
#define MPX_VARIANT_CLOUD_CULL 3
#define MPX_VARIANT_COUNT_ 4
int mpx_set_variant(int what, int value);
int mpx_get_variant(int what); /* -1: unknown selector */

/* Verification hooks (host calls; nothing is launched and no GPU is needed): the kernel form a launcher takes for a call of
 * this shape, as the launcher itself computes it (csrc/launch_routes.h -- every launcher plans with these functions and then
 * dispatches on the plan).  Each writes its fields to `route` (int32, the stated length) and returns 0.
 *
 * mpx_fps_route, route[4]: family (0 plain, 1 wave per environment, 2 Morton-culled with 8 waves, 3 culled with 4 waves),
 * points per lane (the instantiation), threads per workgroup, dynamic LDS bytes.  Reads MPX_VARIANT_FPS as mpx_fps does. */
int mpx_fps_route(int B, int N, int32_t *route);
/* route[6]: form (0 nothing to launch, 1 general, 2 one wave per environment, 3 per-environment 256-thread form), pairs per
 * thread (forms 2, 3: the instantiation), threads per workgroup, waypoints per chunk (forms 2, 3), chunks per environment
 * (form 1: workgroups of the launch), (waypoint, sphere) pairs of the last chunk (form 1: of the last workgroup).
 * frames_aligned: both frame pointers are 16-byte aligned.  The flags-only call takes the same route.                  */
int mpx_franka_collision_route(int B, int T, int S, int M1, int M2, int frames_aligned, int32_t *route);
/* mpx_linear / mpx_linear_ws, route[3]: form (0 gemv, 1 128 x 128 tiles, 2 split-K, taken by mpx_linear_ws with a workspace),
 * slices of K, k per slice.  (mpx_linear's row-per-lane form for N = 128, K = 68 and the DMA staging of the tile kernel
 * also depend on the operands' addresses and strides; they replace form 1 only.)                                        */
int mpx_linear_route(int M, int N, int K, int32_t *route);
/* What mpx_linear would launch for exactly these operands (the same arguments, checked the same way; non-zero where
 * mpx_linear refuses them or M < 1).  form[3]: form[0] as route[0] above; form[1] = 1: the row-per-lane kernel (N = 128,
 * K = 68, no bias, no activation, ldx even, ldy % 4 == 0, x and w 8-byte and y 16-byte aligned, more rows than the gemv
 * form takes); form[2] = 1: the first slab of rows takes the tile kernel and stages its operands by DMA (K % 16 == 0 and
 * operands a 32-bit byte offset spans).  The predicates are the launcher's own.                                          */
int mpx_linear_form(const float *x, int ldx, const float *w, const float *bias, int M, int N, int K, int act,
                    const float *y, int ldy, int32_t *form);
/* mpx_linear_wgrad / _bf16x3, route[3]: tile (64 or 128), splits over the rows (mpx_linear_wgrad_scratch = splits *
 * (N K + N) floats; 1: the gradient is written directly when db follows dw), rows per split.                            */
int mpx_linear_wgrad_route(int M, int N, int K, int32_t *route);
/* mpx_pool_wgrad, route[1]: splits over the queries (mpx_pool_wgrad_scratch = splits * (C K + C) floats).              */
int mpx_pool_wgrad_route(int64_t Q, int C, int K, int32_t *route);
/* The grouped-MLP entries mpx_sa_mlp (bf16x3 0, factored 0), mpx_sa_mlp_factored (0, 1), mpx_sa_mlp_bf16x3 (1, 0) and
 * mpx_sa_mlp_bf16x3_factored (1, 1) on a device of `cus` compute units (<= 0: the current device's own count).  C: the
 * module's feature channels (1 or 64); has_counts: cnt is given; out_aligned: out_stride % 4 == 0 and out 16-byte aligned.
 * route[10]: packed kernel (fp32: the hit counts are honoured), queries per wave (the instantiation), pooling through LDS
 * (fp32, C = 1), units (fp32 packed, bf16x3 factored) or workgroups (the other forms) covering the queries, units /
 * workgroups per environment when whole environments go to one XCD (else 0), persistent grid fed from the unit queue wanted,
 * its workgroups, bf16x3 weight-resident kernel (else lockstep), a wave's queries share their environment (resident),
 * XCD-aware unit order (bf16x3 factored).                                                                               */
int mpx_sa_mlp_route(int cus, int B, int npoint, int nsample, int has_counts, int C, int bf16x3, int factored,
                     int out_aligned, int32_t *route);

/* ball_query: first `nsample` indices (ascending) with d2 < radius^2, padded with the first
 * hit, zero when there is none.  idx int32 [B,npoint,nsample].  cnt (optional, int32
 * [B,npoint]) receives the number of real hits (<= nsample): slots [cnt, nsample) are padding. */
int mpx_ball_query(const float *new_xyz, int new_stride, const float *xyz, int stride, int B,
                   int N, int npoint, float radius, int nsample, int32_t *idx, int32_t *cnt,
                   mpx_stream_t stream);

/* The same search, writing the HIT slots only: idx[b, j, 0 .. max(cnt, 1)) (an empty row still gets its slot 0 = 0); the
 * padding slots are left untouched.  For consumers that take `cnt` and never look past it (mpx_sa_mlp / _factored /
 *  _bf16x3 with counts): most of a row is padding, so most of the index writes go away.  cnt is required; nsample <= 256
 * (the most slots per neighbourhood for which the grouped-MLP kernels honour the counts).                            */
int mpx_ball_query_hits(const float *new_xyz, int new_stride, const float *xyz, int stride, int B,
                        int N, int npoint, float radius, int nsample, int32_t *idx, int32_t *cnt,
                        mpx_stream_t stream);

/* The hit slots as a SET: cnt[b, j] is that of mpx_ball_query, and idx[b, j, 0 .. max(cnt, 1)) holds exactly the indices
 * mpx_ball_query_hits writes there, in UNSPECIFIED order (an empty row gets its slot 0 = 0); every other slot is left
 * untouched.  For consumers that reduce over the listed neighbours with a max and therefore consume no order: the fused
 * grouped-MLP kernels with counts (mpx_sa_mlp / _factored / _bf16x3 / _bf16x3_factored) evaluate each listed neighbour as
 * an independent row and max-pool, so their output is bit-identical to the ordered rows' (max(+0, -0) may be either zero,
 * but relu(x + b3) follows and maps both to the same bits).  A query with more than nsample hits still keeps the nsample
 * SMALLEST indices.  The bucketed search (2048 <= N <= 8192, small radius) hands out slots in arrival order and skips
 * its per-row sort: the ORDER inside a row is not reproducible from run to run; counts, sets and consumers' outputs are.
 * The other search kernels emit index order by construction.  cnt is required; nsample <= 256.                       */
int mpx_ball_query_set(const float *new_xyz, int new_stride, const float *xyz, int stride, int B,
                       int N, int npoint, float radius, int nsample, int32_t *idx, int32_t *cnt,
                       mpx_stream_t stream);

/* order[i] = query ids (0..n-1) sorted by DEcreasing number of rows they contribute to the packed
 * SA kernels, 4*ceil(clamp(cnt,1,nsample)/4) (ties in unspecified order).  scratch: int32[128]
 * device words (zeroed by the call).  Gives the lockstep waves of mpx_sa_mlp_bf16x3 equal work. */
int mpx_sort_queries(const int32_t *cnt, int64_t n, int nsample, int32_t *order, int32_t *scratch,
                     mpx_stream_t stream);

/* QueryAndGroup (use_xyz=True) materialised like the reference does:
 * out [B, 3+C, npoint, nsample]; feat point-major rows at feat + (b*N+k)*feat_stride.       */
int mpx_group_points(const float *xyz, int stride, const float *new_xyz, int new_stride,
                     const float *feat, int feat_stride, int C, const int32_t *idx, int B, int N,
                     int npoint, int nsample, float *out, mpx_stream_t stream);

/* Fused QueryAndGroup + shared MLP (3 x [1x1 conv + ReLU]) + max-pool over the neighbourhood
 * (PointnetSAModule.forward body), fp32 MFMA, nothing materialised in HBM.
 * Channel order of the MLP input is [dx,dy,dz, feat...] like the reference.
 * wpack: weights + biases packed by mpx_sa_pack_weights for this (C, c1, c2, c3).
 * out rows at out + (b*npoint + j)*out_stride, c3 floats each.
 * Supported: (C,c1,c2,c3) = (1,64,64,64) and (64,128,128,256); nsample % 32 == 0.
 * cnt (optional, from mpx_ball_query): only the DISTINCT neighbours are evaluated -- slots
 * [cnt, nsample) repeat the first neighbour, the MLP is per point and max-pooling is idempotent,
 * so the output is bit-identical to walking all nsample slots (cnt == NULL).  Several queries
 * share a wave and their rows are packed (rounded up to 2 rows per query for the narrow module, 4 for the
 * wide one) into the 32-row MFMA tiles.  Large launches with cnt are PERSISTENT: one workgroup per wave slot
 * of the chip takes units of consecutive queries from the device-side queue described at
 * mpx_sa_mlp_bf16x3_factored_wants_order below (same per-(device, stream) counters, same hipGraph note).
 * append_centre != 0 (needs cnt, out_stride >= c3 + 4): columns [c3, c3+3) of every output row also receive the
 * query point's coordinates and column c3+3 a zero -- the rows are then the operand [f | xyz | 0] of the next
 * module's per-point first-layer GEMM (mpx_sa_mlp_factored), model.py:404-407's torch.cat without a second pass. */
int mpx_sa_mlp(const float *xyz, int stride, const float *new_xyz, int new_stride,
               const float *feat, int feat_stride, int C, const int32_t *idx, const int32_t *cnt,
               int B, int N, int npoint, int nsample, const float *wpack, int c1, int c2, int c3,
               float *out, int out_stride, int append_centre, mpx_stream_t stream);
/* Same module with the first layer factored out of the per-(query, neighbour) work:
 *   W1.[p_j - c_i ; f_j] + b1 = pre[j] - ctr[i],  pre = [p ; f].W1^T  (one row per POINT, [B*N, c1]),
 *                                                 ctr = c.W1x^T - b1  (one row per QUERY, [B*npoint, c1]),
 * both plain mpx_linear calls by the caller.  The kernel gathers pre rows, subtracts the query row,
 * applies ReLU and continues with layers 2-3 and the max-pool as above (wpack unchanged; its layer-1
 * block is not read).  15 % less matrix work for the (64,128,128,256) module; equal to mpx_sa_mlp
 * up to the rounding of that one re-associated sum.  cnt is required.  (Persistent for large launches, as above.) */
int mpx_sa_mlp_factored(const float *pre, const float *ctr, const int32_t *idx, const int32_t *cnt, int B,
                        int N, int npoint, int nsample, const float *wpack, int C, int c1, int c2, int c3,
                        float *out, int out_stride, mpx_stream_t stream);
/* mpx_sa_mlp_factored on the bf16 matrix cores (split products, see mpx_sa_mlp_bf16x3): wpack from
 * mpx_sa_pack_bf16x3 (its layer-1 blocks are not read); order (optional) from mpx_sort_queries.
 * nsample <= 128 (the kernel's row -> query table is sized for it; larger neighbourhoods are refused). */
/* host query: does mpx_sa_mlp_bf16x3_factored use `order`?  Always 0 since version 300: its one kernel is persistent
 * and takes units of 8 queries from a device-side queue (`order` is ignored; pass NULL).  The queue is 32 bytes of
 * library-image memory per (device, stream), zeroed on the launch stream in front of the kernel: concurrent calls on
 * DIFFERENT streams never share counters (up to 256 streams per process).  hipGraph: a captured call bakes its capture
 * stream's queue in -- do not replay two graphs that were captured on the same stream concurrently on two streams.   */
int mpx_sa_mlp_bf16x3_factored_wants_order(void);
int mpx_sa_mlp_bf16x3_factored(const float *pre, const float *ctr, const int32_t *idx, const int32_t *cnt,
                               const int32_t *order, int B, int N, int npoint, int nsample, const void *wpack,
                               int C, int c1, int c2, int c3, float *out, int out_stride, mpx_stream_t stream);
/* number of floats mpx_sa_pack_weights writes for this configuration (host call)            */
int64_t mpx_sa_pack_size(int C, int c1, int c2, int c3);
/* w1 [c1,3+C], w2 [c2,c1], w3 [c3,c2] row-major (Conv2d 1x1 weights), b* biases -> wpack    */
int mpx_sa_pack_weights(const float *w1, const float *b1, const float *w2, const float *b2,
                        const float *w3, const float *b3, int C, int c1, int c2, int c3,
                        float *wpack, mpx_stream_t stream);

/* Split-bf16 ("bf16x3") variant of mpx_sa_mlp: every fp32 product is evaluated as
 * x_hi*w_hi + x_hi*w_lo + x_lo*w_hi on the bf16 matrix cores with fp32 accumulation (5.3x fewer
 * MFMA cycles; |error| ~ 2^-16 relative per product, ~3e-7 on the policy output).  Same arguments
 * and outputs as mpx_sa_mlp; wpack comes from mpx_sa_pack_bf16x3 (size in BYTES from
 * mpx_sa_pack_bf16x3_size).  Opt-in: the fp32 kernel is the parity default.  cnt as in mpx_sa_mlp
 * (distinct neighbours only, rows packed; NULL = all slots).  `order` (optional, from
 * mpx_sort_queries) is the order in which waves take the queries: the 8 waves of a workgroup walk
 * the weight stream in lockstep and run max(tiles) of their row counts.  A module whose whole pack fits
 * LDS (the first one, 1+3 -> 64 -> 64 -> 64) runs a weight-resident kernel instead that takes the queries
 * in their natural order (up to nsample = 128): mpx_sa_mlp_bf16x3_wants_order (host query; the launcher uses the
 * same predicate) says whether `order` is used for a module and neighbourhood size.  append_centre as in mpx_sa_mlp
 * (only where `order` is not used).                                                                        */
int mpx_sa_mlp_bf16x3_wants_order(int C, int c1, int c2, int c3, int nsample);
int mpx_sa_mlp_bf16x3(const float *xyz, int stride, const float *new_xyz, int new_stride,
                      const float *feat, int feat_stride, int C, const int32_t *idx,
                      const int32_t *cnt, const int32_t *order, int B, int N, int npoint,
                      int nsample, const void *wpack, int c1, int c2, int c3, float *out,
                      int out_stride, int append_centre, mpx_stream_t stream);
int64_t mpx_sa_pack_bf16x3_size(int C, int c1, int c2, int c3);
int mpx_sa_pack_bf16x3(const float *w1, const float *b1, const float *w2, const float *b2,
                       const float *w3, const float *b3, int C, int c1, int c2, int c3, void *wpack,
                       mpx_stream_t stream);

/* The group-all set-abstraction module (PointnetSAModule(mlp=[256(+3), 512, 512, 1024]), npoint = None: model.py:377-383)
 * as ONE kernel: x rows [B*rows, K1] (ldx floats apart; [xyz | features | 0], K1 = 272 = 259 padded to whole 16-float
 * slabs), rows = 128 per environment -> Linear + ReLU (K1 -> c1) -> Linear + ReLU (c1 -> c2) -> Linear + ReLU (c2 -> c3)
 * -> max over the environment's rows -> out [B, c3] (ldo floats apart).  Nothing between the input rows and the pooled row
 * touches HBM (the layer-by-layer form writes and re-reads two [B*128, 512] intermediates).  fp32 MFMA, exact fp32
 * products; the summation order inside a dot product differs from mpx_linear's (1e-7 relative).  One workgroup per
 * environment: meant for B >= 256.  pack: mpx_sa3_pack_weights (size in floats: mpx_sa3_pack_size; -1 = unsupported
 * shape; supported: (K1, c1, c2, c3) = (272, 512, 512, 1024)); w1 is [c1, k1_real] row-major with k1_real <= K1 real
 * input columns (259), w2 [c2, c1], w3 [c3, c2].                                                                       */
int64_t mpx_sa3_pack_size(int K1, int c1, int c2, int c3);
int mpx_sa3_pack_weights(const float *w1, int k1_real, const float *b1, const float *w2, const float *b2, const float *w3,
                         const float *b3, int K1, int c1, int c2, int c3, float *pack, mpx_stream_t stream);
int mpx_sa3_chain(const float *x, int ldx, int B, int rows, const float *pack, int K1, int c1, int c2, int c3, float *out,
                  int ldo, mpx_stream_t stream);

/* ---- dense layers: model.py:47-66, 385-393 ------------------------------------------------- */

#define MPX_ACT_NONE 0
#define MPX_ACT_RELU 1
#define MPX_ACT_LEAKY 2 /* slope 0.01, nn.LeakyReLU() default */

/* y[m, n] = act(sum_k x[m,k] * w[n,k] + bias[n]);  x rows at x + m*ldx, y rows at y + m*ldy.
 * fp32 MFMA.  K % 4 == 0, ldx % 4 == 0, x and w 16-byte aligned.                             */
int mpx_linear(const float *x, int ldx, const float *w, const float *bias, int M, int N, int K,
               int act, float *y, int ldy, mpx_stream_t stream);

/* The same layer with a caller-provided workspace that lets skinny problems (few 128x128 output tiles, long K:
 * the fc / decoder layers of a single-problem or few-hundred-problem rollout) split K over the chip's CUs.
 * mpx_linear_workspace(M,N,K) = bytes this shape wants (0: it would not split); the partial sums are added in
 * slice order, so results are deterministic (they differ from mpx_linear's by fp32 summation order only).
 * workspace == NULL behaves exactly like mpx_linear.                                          */
int64_t mpx_linear_workspace(int M, int N, int K);
int mpx_linear_ws(const float *x, int ldx, const float *w, const float *bias, int M, int N, int K,
                  int act, float *y, int ldy, void *workspace, int64_t workspace_bytes,
                  mpx_stream_t stream);

/* Last layer of the group-all SA module with its max-pool fused (model.py:383):
 *   y[g, n] = max over the `rows` rows of group g of relu(x[g*rows + r, :] . w[n, :] + bias[n])
 * rows must be 128 (one workgroup tile) and divide M; y [M/rows, N] is written (zeroed first).  */
int mpx_linear_rowmax(const float *x, int ldx, const float *w, const float *bias, int M, int N,
                      int K, int rows, float *y, int ldy, mpx_stream_t stream);

/* nn.GroupNorm(groups, C) (eps 1e-5, biased variance) followed by LeakyReLU(0.01), in place
 * allowed.  x,y [M,C].                                                                       */
int mpx_groupnorm_leaky(const float *x, const float *gamma, const float *beta, int M, int C,
                        int groups, float eps, float *y, mpx_stream_t stream);
/* the same, with the result written in the bf16x3 dense layers' pairs form (see mpx_split_bf16; C a multiple of
 * 16, ldp >= 2 C bf16 elements) instead of fp32 rows: the operand of the dense layer that follows.  */
int mpx_groupnorm_leaky_to_pairs(const float *x, const float *gamma, const float *beta, int M, int C,
                                 int groups, float eps, void *y_pairs, int ldp, mpx_stream_t stream);

/* max over `rows` consecutive rows: x [G*rows, C] -> y [G, C]  (max_pool2d of the group-all
 * SA module, model.py:383)                                                                   */
int mpx_rowmax(const float *x, int ldx, int G, int rows, int C, float *y, int ldy,
               mpx_stream_t stream);

/* rows[i, col0 : col0+ncols] = src[i, :ncols] and rows[i, col0+ncols : col0+ncols+nzero] = 0 for i < n (strides in
 * floats).  Builds SA2's per-point operand rows [f1 | xyz1 | 0] next to the features SA1 wrote (model.py:404-407's
 * torch.cat of xyz and features, without the copy of the features).                                              */
int mpx_append_columns(const float *src, int src_stride, int ncols, int nzero, int64_t n, float *rows,
                       int row_stride, int col0, mpx_stream_t stream);

/* ---- the whole policy forward in one call: MotionPolicyNetwork.forward, model.py:75-91 ------------------------
 * For callers without Python (a native planning node): slab + joint configuration in, displacement out.  Host-side
 * orchestration of the kernels above in the order and shapes of mpinets_amd/model.py, whose fp32 output it
 * reproduces bit for bit; the caller's stream (for B <= 512 also an internal second stream, forked and joined with
 * events -- hipGraph-capturable; concurrent calls from several host threads on one device are safe: the internal
 * stream is held exclusively from fork to join), no allocation, no synchronisation.
 *
 * Weights: device pointers, fp32, [out, in] row-major like nn.Linear / 1x1 Conv2d, prepared once:
 *   sa1_pack, sa2_pack   mpx_sa_pack_weights of SA_modules.{0,1} (C = 1 and 64)
 *   sa2_wpoint [128,68]  SA2's first layer over rows [f1 (64) | xyz (3) | 0]   (W1[:,3:] | W1[:,:3] | 0)
 *   sa2_wcentre [128,4]  ... over rows [xyz (3) | *]                             (W1[:,:3] | 0)
 *   sa2_nb1 [128]        minus its bias
 *   sa3_w[0] [512,272]   group-all first layer, K padded 259 -> 272 with zero columns; sa3_w[1] [512,512];
 *                        sa3_w[2] [1024,512]; sa3_b[i] the biases (the layer-by-layer form: B < 256 problems)
 *   sa3_pack             the same three layers packed by mpx_sa3_pack_weights (the fused form: B >= 256); NULL: the
 *                        layer-by-layer form at every batch size (same results within rounding)
 *   fc_w / fc_b          1024 -> 4096 -> 2048 -> 2048; gn_g / gn_b: the two GroupNorm(16) affine vectors
 *   qe_w[0] [32,8]       joint encoder, first layer K padded 7 -> 8; then 32 -> 64 -> 128 -> 128 -> 64
 *   de_w / de_b          decoder 2112 -> 512 -> 256 -> 128 -> 7                                                  */
typedef struct mpx_policy_weights {
  const float *sa1_pack, *sa2_pack, *sa2_wpoint, *sa2_wcentre, *sa2_nb1;
  const float *sa3_w[3], *sa3_b[3];
  const float *fc_w[3], *fc_b[3], *gn_g[2], *gn_b[2];
  const float *qe_w[5], *qe_b[5];
  const float *de_w[4], *de_b[4];
  const float *sa3_pack; /* mpx_sa3_pack_weights of the group-all module (K1 = 272): the fused chain of B >= 256 problems, or NULL */
} mpx_policy_weights;

/* bytes of 256-byte aligned device workspace a batch of B problems with N-point slabs needs */
int64_t mpx_policy_workspace(int B, int N);
/* xyz [B,N,4] (x, y, z, label; N in [512, 8192]), q [B,7] normalised to [-1,1] -> dq [B,7] (normalised space).
 * B <= 65535.                                                                                                    */
int mpx_policy_forward(const mpx_policy_weights *w, const float *xyz, int N, const float *q, int B,
                       float *dq, void *workspace, int64_t workspace_bytes, mpx_stream_t stream);

/* Per-call robot-point subset.  robofin's FrankaSampler.sample redraws np.random.choice(P, num_points, replace=False) on
 * EVERY call, ONE subset shared by the batch (call sites mpinets/model.py:170-181, run_inference.py:188-189); NumPy's
 * global RNG cannot be reproduced on a device, so the distribution is what is kept: out int32 [n_out] <- n_out of the
 * `total` table rows, uniformly without replacement, in uniform order (row i keyed by Philox4x32-10 with counter
 * (i >> 2, draw, 11, 0) and key `seed`; the n_out smallest (key, row) pairs in that order).  n_out <= 4096.  Depends on
 * (seed, draw) only: every rank of a sharded batch draws the same subset, like one process would.                 */
int mpx_draw_subset(int total, int n_out, uint64_t seed, int draw, int32_t *out, mpx_stream_t stream);

/* ---- closed-loop steps in one call: TrainingMotionPolicyNetwork.rollout's loop body (model.py:160-181) plus the
 * collision check of validation_step (model.py:293-314), i.e. what mpinets_amd.rollout.RolloutEngine.step() does
 * with a static scene:  dq = policy(xyz, q_norm);  q_norm = clamp(q_norm + dq, -1, 1);  q = unnormalise(q_norm);
 * robot rows of the slab <- FK cloud of q;  flags = any collision sphere of q inside a primitive.
 * Everything besides the policy weights that the step reads (device pointers, shared by the batch unless noted): */
typedef struct mpx_rollout_scene {
  const float *limits;           /* [7,2] joint limits (lower, upper)                                            */
  float finger;                  /* prismatic finger opening used for FK                                        */
  const float *table_pts;        /* FrankaSampler point table [P,3] in link frames ...                         */
  const int32_t *table_link;     /* ... and the link of each point [P]                                         */
  const int32_t *subset;         /* the n_robot table rows written to the slab (NULL: the first n_robot)       */
  int n_robot;                   /* robot rows at the head of every slab (2048)                                */
  const float *sph_centers, *sph_radii; /* collision spheres [S,3], [S] in link frames ...                     */
  const int32_t *sph_link;       /* ... and their links [S]                                                    */
  int n_spheres;
  const float *cub_frames, *cub_dims;   /* per environment: [B,M1,4,4] inverse frames (mpx_prim_frames), [B,M1,3] */
  int M1;
  const float *cyl_frames, *cyl_radii, *cyl_heights;   /* [B,M2,4,4], [B,M2], [B,M2]                           */
  int M2;
} mpx_rollout_scene;

/* What a multi-step rollout does besides the plain step (all optional; a zeroed struct with steps = 1 is
 * mpx_rollout_step): the engine-side form of rollout_until_success's loop body (run_inference.py:171-189) and of
 * the "closed-loop point-cloud re-render" workload.                                                              */
typedef struct mpx_rollout_options {
  int steps;                      /* closed-loop steps to enqueue (no host synchronisation in between)            */
  int first_step;                 /* index of the first of them: the re-render seed schedule continues an earlier call */
  /* scene re-render at the start of every step (n_scene = 0: the scene rows of the slab stay as they are):
   * n_scene points per environment drawn from the scene's primitives by mpx_scene_cloud with seed
   * scene_seed + 7919 * step and global environment ids env_offset + row, written to slab rows
   * [n_robot, n_robot + n_scene).  Needs the primitives' raw poses beside the frames in mpx_rollout_scene.      */
  int n_scene;
  uint64_t scene_seed;
  int64_t env_offset;
  const float *cub_centers, *cub_quats;   /* [B,M1,3], [B,M1,4] (w,x,y,z) */
  const float *cyl_centers, *cyl_quats;   /* [B,M2,3], [B,M2,4]           */
  /* success tracking (target_poses = NULL: off): after every joint update, environments whose right_gripper is
   * within pos_tol metres and cos_rot_tol (cosine of the angle) of target_poses [B,4,4] set done[b] (int32 [B],
   * zeroed by the caller before the first call) and keep their configuration from then on; steps_taken (optional,
   * int32 [B], zeroed by the caller) counts the policy steps each environment took until it was done.          */
  const float *target_poses;
  float pos_tol, cos_rot_tol;
  int32_t *done, *steps_taken;
  /* optional [B, trajectory_len, 7]: waypoint trajectory_row + i of every environment receives q after step i of
   * this call (row 0 is normally the caller's start configuration, so the first call passes trajectory_row = 1)  */
  float *trajectory;
  int trajectory_len, trajectory_row;
  /* per-step robot-point subset (subset_table_size = 0: off, the scene's fixed `subset` is used): before the FK cloud
   * refresh of step s, subset_buf (int32 [n_robot], caller's device buffer) <- mpx_draw_subset(subset_table_size,
   * n_robot, subset_seed, s) and the refresh writes THOSE table rows -- the reference's per-call redraw.         */
  int subset_table_size;
  uint64_t subset_seed;
  int32_t *subset_buf;
} mpx_rollout_options;

/* workspace bytes (256-byte aligned) of mpx_rollout / mpx_rollout_step */
int64_t mpx_rollout_workspace(int B, int N);
/* xyz [B,N,4] slab (robot rows -- and scene rows when re-rendering -- rewritten in place), q_norm [B,7] in/out,
 * q [B,7] out (radians), flags int32 [B] OR-ed into (non-zero: some step's configuration was in collision),
 * min_sdf [B, n_spheres] out or NULL (last step's).  Bit-identical to RolloutEngine.step() called `steps` times.  */
int mpx_rollout(const mpx_policy_weights *w, const mpx_rollout_scene *scene, const mpx_rollout_options *options,
                float *xyz, int N, float *q_norm, float *q, int B, int32_t *flags, float *min_sdf, void *workspace,
                int64_t workspace_bytes, mpx_stream_t stream);
/* one plain step (static scene, no success tracking): mpx_rollout with a zeroed options struct and steps = 1 */
int mpx_rollout_step(const mpx_policy_weights *w, const mpx_rollout_scene *scene, float *xyz, int N,
                     float *q_norm, float *q, int B, int32_t *flags, float *min_sdf, void *workspace,
                     int64_t workspace_bytes, mpx_stream_t stream);

/* ---- measurement hooks (the scripts under tools/probes; no product path calls them) ------------------------------------------
 * The same launches as mpx_sa3_chain / mpx_sa_mlp_bf16x3_factored through instantiations that write s_memtime stamps
 * of one wave at the kernel's phase boundaries.                                                                    */
/* probe: int64 [>= 32]; B >= 301 (workgroup 300's wave 0 is the one stamped) */
int mpx_sa3_chain_probe(const float *x, int ldx, int B, const float *pack, float *out, int ldo, int64_t *probe,
                        mpx_stream_t stream);
/* probe: int64 [>= 128] or NULL (off): while set, every mpx_sa_mlp_bf16x3_factored call first runs the stamped
 * instantiation (process-wide switch, not thread-safe) */
int mpx_sa2_bf16x3_set_probe(int64_t *probe);
/* mpx_sa3_front_bf16x3 with stamps (probe: int64 [>= 64]; B > 300) */
int mpx_sa3_front_bf16x3_probe(const float *x, int ldx, int B, const void *pack, void *y_pairs, int ldp, int64_t *probe,
                               mpx_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MPINETS_HIP_H */
