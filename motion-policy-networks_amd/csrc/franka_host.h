// franka_host.h -- host-only (no __device__ code): the option defaults, the argument checks and the cloud launch table that
// the Franka geometry entries share (ik.hip, plan.hip, roadmap.hip, gripper_roadmap.hip, task_candidates.hip, follow.hip, cloud_collision.hip, cloud_field.hip; cloud_clean.hip for
// env_offset and scratch size); a new entry takes its defaults and its checks from here, and states a refusal of its own only
// where no other entry has it.  Each takes the name of the entry the caller invoked, reports through MPX_REQUIRE and
// returns 0 or 1 (field_grid_check's idiom).  Sizes and values are checked before an entry's "nothing to do" return, pointers after.
#pragma once
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <type_traits>

#include "common.h"

// options: the defaults (MPX_*_DEFAULT_*, include/mpinets_hip.h) and what a kernel can run with
static inline mpx_ik_options franka_ik_defaults() {
  return {MPX_IK_DEFAULT_ITERATIONS, MPX_IK_DEFAULT_LAMBDA, MPX_IK_DEFAULT_STEP_CLIP, MPX_IK_DEFAULT_POS_TOL,
          MPX_IK_DEFAULT_ROT_TOL, 0.0f, 0};
}
static inline mpx_plan_options franka_plan_defaults() {
  return {MPX_PLAN_DEFAULT_CANDIDATES, MPX_PLAN_DEFAULT_ITERATIONS, MPX_PLAN_DEFAULT_STEP, MPX_PLAN_DEFAULT_SMOOTH_WEIGHT,
          MPX_PLAN_DEFAULT_EPSILON, MPX_PLAN_DEFAULT_SPREAD, MPX_PLAN_DEFAULT_SUBSTEPS, MPX_PLAN_DEFAULT_CHECK_MARGIN, 0.0f,
          MPX_PLAN_DEFAULT_MAX_JERK, 1};
}
static inline mpx_roadmap_options franka_roadmap_defaults() {
  return {MPX_ROADMAP_DEFAULT_NODES, MPX_ROADMAP_DEFAULT_RESOLUTION, __builtin_inff(), MPX_ROADMAP_DEFAULT_MAX_ROUNDS,
          MPX_ROADMAP_DEFAULT_SMOOTH_PASSES, MPX_PLAN_DEFAULT_CHECK_MARGIN, 0.0f, 1};
}
static inline mpx_shortcut_options franka_shortcut_defaults() {
  return {MPX_SHORTCUT_DEFAULT_POINTS, MPX_SHORTCUT_DEFAULT_PASSES, MPX_SHORTCUT_DEFAULT_FANOUT, MPX_ROADMAP_DEFAULT_RESOLUTION,
          MPX_ROADMAP_DEFAULT_SMOOTH_PASSES, MPX_PLAN_DEFAULT_CHECK_MARGIN, 0.0f, 1};
}
static inline mpx_gripper_roadmap_options gripper_roadmap_defaults() {
  return {MPX_GRIPPER_ROADMAP_DEFAULT_NODES, MPX_GRIPPER_ROADMAP_DEFAULT_RESOLUTION, MPX_GRIPPER_ROADMAP_DEFAULT_ROT_WEIGHT,
          MPX_GRIPPER_ROADMAP_DEFAULT_ORIENT_SPREAD, __builtin_inff(), MPX_GRIPPER_ROADMAP_DEFAULT_MAX_ROUNDS,
          MPX_PLAN_DEFAULT_CHECK_MARGIN, 0.0f, 1};
}
static inline mpx_gripper_shortcut_options gripper_shortcut_defaults() {
  return {MPX_SHORTCUT_DEFAULT_POINTS, MPX_SHORTCUT_DEFAULT_PASSES, MPX_SHORTCUT_DEFAULT_FANOUT,
          MPX_GRIPPER_ROADMAP_DEFAULT_RESOLUTION, MPX_GRIPPER_ROADMAP_DEFAULT_ROT_WEIGHT, MPX_PLAN_DEFAULT_CHECK_MARGIN, 0.0f, 1};
}
static inline mpx_task_candidates_options task_candidates_defaults() { return {MPX_TASK_DEFAULT_DRAWS, 0.0f, 1, 0.0f, 0}; }
static inline mpx_follow_options franka_follow_defaults() {
  return {MPX_FOLLOW_DEFAULT_DT, MPX_FOLLOW_DEFAULT_MAX_STEPS, MPX_FOLLOW_DEFAULT_ATTRACT, MPX_FOLLOW_DEFAULT_DAMPING,
          MPX_IK_DEFAULT_LAMBDA, MPX_IK_DEFAULT_STEP_CLIP, MPX_FOLLOW_DEFAULT_REPEL, MPX_PLAN_DEFAULT_EPSILON, 0.0f,
          MPX_FOLLOW_DEFAULT_LIMIT_GAIN, MPX_FOLLOW_DEFAULT_LIMIT_BAND, MPX_FOLLOW_DEFAULT_SPEED_LIMIT,
          MPX_FOLLOW_DEFAULT_SWITCH_RADIUS, MPX_FOLLOW_DEFAULT_SWITCH_STEPS, MPX_FOLLOW_DEFAULT_FINAL_RADIUS,
          MPX_FOLLOW_DEFAULT_FINAL_STEPS, MPX_PLAN_DEFAULT_SUBSTEPS, MPX_PLAN_DEFAULT_CHECK_MARGIN, MPX_PLAN_DEFAULT_MAX_JERK, 1,
          MPX_FOLLOW_DEFAULT_MISS_TOL};
}
static inline int franka_ik_options_check(const char *who, const mpx_ik_options &opt) {
  MPX_REQUIRE(opt.iterations >= 1, "%s: iterations = %d, need >= 1", who, opt.iterations);
  MPX_REQUIRE(opt.lambda > 0.0f, "%s: lambda must be > 0 (the 6x6 solve has no pivoting)", who);
  MPX_REQUIRE(opt.step_clip > 0.0f, "%s: step_clip must be > 0", who);
  MPX_REQUIRE(opt.pos_tol >= 0.0f && opt.rot_tol >= 0.0f, "%s: negative tolerance", who);
  MPX_REQUIRE(opt.clearance == opt.clearance, "%s: clearance is NaN", who);
  return 0;
}
// (the three sizes a planner's LDS and scratch layouts are computed from: mpx_franka_plan_cloud_scratch asks them too)
static inline bool franka_plan_T_ok(int T) { return T >= 2 && T <= MPX_PLAN_MAX_T; }
static inline bool franka_plan_candidates_ok(int K) { return K >= 1 && K <= MPX_PLAN_MAX_CANDIDATES; }
static inline bool franka_plan_substeps_ok(int substeps) { return substeps >= 1 && substeps <= 64; }
static inline int franka_plan_T_check(const char *who, int T) {
  MPX_REQUIRE(franka_plan_T_ok(T), "%s: T = %d waypoints, need 2 .. %d (one lane each)", who, T, MPX_PLAN_MAX_T);
  return 0;
}
static inline int franka_plan_options_check(const char *who, int T, const mpx_plan_options &opt) {
  if (franka_plan_T_check(who, T)) return 1;
  MPX_REQUIRE(franka_plan_candidates_ok(opt.candidates), "%s: candidates = %d, need 1 .. %d (one wave each)", who,
              opt.candidates, MPX_PLAN_MAX_CANDIDATES);
  MPX_REQUIRE(opt.iterations >= 0, "%s: iterations = %d, need >= 0", who, opt.iterations);
  MPX_REQUIRE(opt.step > 0.0f, "%s: step must be > 0", who);
  MPX_REQUIRE(opt.epsilon > 0.0f, "%s: epsilon must be > 0", who);
  MPX_REQUIRE(opt.smooth_weight >= 0.0f, "%s: smooth_weight must be >= 0", who);
  MPX_REQUIRE(franka_plan_substeps_ok(opt.substeps), "%s: substeps = %d, need 1 .. 64", who, opt.substeps);
  MPX_REQUIRE(opt.check_margin >= 0.0f && opt.max_jerk >= 0.0f, "%s: negative check_margin or max_jerk", who);
  MPX_REQUIRE(opt.clearance == opt.clearance && opt.spread == opt.spread, "%s: clearance or spread is NaN", who);
  return 0;
}
// (every float is tested as `x >= 0` or `x > 0`: a NaN fails either)
static inline int franka_follow_options_check(const char *who, int W, int T, const mpx_follow_options &opt) {
  if (franka_plan_T_check(who, T)) return 1;
  MPX_REQUIRE(W >= 1 && W <= MPX_FOLLOW_MAX_POSES, "%s: W = %d guide poses, need 1 .. %d", who, W, MPX_FOLLOW_MAX_POSES);
  MPX_REQUIRE(opt.max_steps >= 1 && opt.max_steps <= MPX_FOLLOW_MAX_STEPS, "%s: max_steps = %d, need 1 .. %d (the time loop's bound)",
              who, opt.max_steps, MPX_FOLLOW_MAX_STEPS);
  MPX_REQUIRE(opt.dt > 0.0f && opt.dt < __builtin_inff(), "%s: dt must be > 0 and finite", who);
  MPX_REQUIRE(opt.lambda > 0.0f, "%s: lambda must be > 0 (the 6x6 solve has no pivoting)", who);
  MPX_REQUIRE(opt.step_clip > 0.0f, "%s: step_clip must be > 0", who);
  MPX_REQUIRE(opt.attract >= 0.0f && opt.damping >= 0.0f && opt.repel >= 0.0f && opt.limit_gain >= 0.0f && opt.limit_band >= 0.0f,
              "%s: negative (or NaN) attract, damping, repel, limit_gain or limit_band", who);
  MPX_REQUIRE(opt.epsilon > 0.0f, "%s: epsilon must be > 0", who);
  MPX_REQUIRE(opt.speed_limit > 0.0f, "%s: speed_limit must be > 0", who);
  MPX_REQUIRE(opt.switch_radius >= 0.0f && opt.final_radius >= 0.0f && opt.miss_tol >= 0.0f,
              "%s: negative (or NaN) switch_radius, final_radius or miss_tol", who);
  MPX_REQUIRE(opt.switch_steps >= 1 && opt.final_steps >= 1, "%s: switch_steps = %d, final_steps = %d, need >= 1", who,
              opt.switch_steps, opt.final_steps);
  MPX_REQUIRE(franka_plan_substeps_ok(opt.substeps), "%s: substeps = %d, need 1 .. 64", who, opt.substeps);
  MPX_REQUIRE(opt.check_margin >= 0.0f && opt.max_jerk >= 0.0f, "%s: negative check_margin or max_jerk", who);
  MPX_REQUIRE(opt.clearance == opt.clearance, "%s: clearance is NaN", who);
  return 0;
}
static inline int franka_roadmap_options_check(const char *who, int T, const mpx_roadmap_options &opt) {
  if (franka_plan_T_check(who, T)) return 1;
  MPX_REQUIRE(opt.nodes >= 2 && opt.nodes <= MPX_ROADMAP_MAX_NODES, "%s: nodes = %d, need 2 .. %d (one thread each)", who,
              opt.nodes, MPX_ROADMAP_MAX_NODES);
  MPX_REQUIRE(opt.resolution > 0.0f, "%s: resolution must be > 0", who);
  MPX_REQUIRE(opt.connect_radius == opt.connect_radius, "%s: connect_radius is NaN", who);
  MPX_REQUIRE(opt.max_rounds >= 1, "%s: max_rounds = %d, need >= 1", who, opt.max_rounds);
  MPX_REQUIRE(opt.smooth_passes >= 0, "%s: smooth_passes = %d, need >= 0", who, opt.smooth_passes);
  MPX_REQUIRE(opt.check_margin >= 0.0f, "%s: negative check_margin", who);
  MPX_REQUIRE(opt.clearance == opt.clearance, "%s: clearance is NaN", who);
  return 0;
}
// (Pin: the rows of the caller's polylines; a thread per vertex and per dense point, so both stay within the roadmap's nodes)
static inline int franka_shortcut_options_check(const char *who, int T, int Pin, const mpx_shortcut_options &opt) {
  if (franka_plan_T_check(who, T)) return 1;
  MPX_REQUIRE(Pin >= 2 && Pin <= MPX_ROADMAP_MAX_NODES, "%s: Pin = %d vertices per polyline, need 2 .. %d (one thread each)", who,
              Pin, MPX_ROADMAP_MAX_NODES);
  MPX_REQUIRE(opt.points >= Pin && opt.points <= MPX_ROADMAP_MAX_NODES, "%s: points = %d, need Pin = %d .. %d (one thread each)",
              who, opt.points, Pin, MPX_ROADMAP_MAX_NODES);
  MPX_REQUIRE(opt.passes >= 0, "%s: passes = %d, need >= 0", who, opt.passes);
  MPX_REQUIRE(opt.fanout >= 1 && opt.fanout <= MPX_SHORTCUT_MAX_FANOUT, "%s: fanout = %d, need 1 .. %d", who, opt.fanout,
              MPX_SHORTCUT_MAX_FANOUT);
  MPX_REQUIRE(opt.resolution > 0.0f, "%s: resolution must be > 0", who);
  MPX_REQUIRE(opt.smooth_passes >= 0, "%s: smooth_passes = %d, need >= 0", who, opt.smooth_passes);
  MPX_REQUIRE(opt.check_margin >= 0.0f, "%s: negative check_margin", who);
  MPX_REQUIRE(opt.clearance == opt.clearance, "%s: clearance is NaN", who);
  return 0;
}
// (W: the guide poses it writes are mpx_franka_follow's operand, so its range is the follower's)
static inline int gripper_roadmap_options_check(const char *who, int W, const mpx_gripper_roadmap_options &opt) {
  MPX_REQUIRE(W >= 1 && W <= MPX_FOLLOW_MAX_POSES, "%s: W = %d guide poses, need 1 .. %d (one thread each)", who, W,
              MPX_FOLLOW_MAX_POSES);
  MPX_REQUIRE(opt.nodes >= 2 && opt.nodes <= MPX_ROADMAP_MAX_NODES, "%s: nodes = %d, need 2 .. %d (one thread each)", who,
              opt.nodes, MPX_ROADMAP_MAX_NODES);
  MPX_REQUIRE(opt.resolution > 0.0f, "%s: resolution must be > 0", who);
  MPX_REQUIRE(opt.rot_weight > 0.0f && opt.rot_weight < __builtin_inff(), "%s: rot_weight must be > 0 and finite", who);
  MPX_REQUIRE(opt.orient_spread >= 0.0f && opt.orient_spread < __builtin_inff(), "%s: orient_spread must be >= 0 and finite", who);
  MPX_REQUIRE(opt.connect_radius == opt.connect_radius, "%s: connect_radius is NaN", who);
  MPX_REQUIRE(opt.max_rounds >= 1, "%s: max_rounds = %d, need >= 1", who, opt.max_rounds);
  MPX_REQUIRE(opt.check_margin >= 0.0f, "%s: negative check_margin", who);
  MPX_REQUIRE(opt.clearance == opt.clearance, "%s: clearance is NaN", who);
  return 0;
}
// (the shortcut's sizes in mpx_franka_shortcut's words, W and rot_weight in mpx_gripper_roadmap's)
static inline int gripper_shortcut_options_check(const char *who, int W, int Pin, const mpx_gripper_shortcut_options &opt) {
  MPX_REQUIRE(W >= 1 && W <= MPX_FOLLOW_MAX_POSES, "%s: W = %d guide poses, need 1 .. %d (one thread each)", who, W,
              MPX_FOLLOW_MAX_POSES);
  MPX_REQUIRE(Pin >= 2 && Pin <= MPX_ROADMAP_MAX_NODES, "%s: Pin = %d vertices per polyline, need 2 .. %d (one thread each)", who,
              Pin, MPX_ROADMAP_MAX_NODES);
  MPX_REQUIRE(opt.points >= Pin && opt.points <= MPX_ROADMAP_MAX_NODES, "%s: points = %d, need Pin = %d .. %d (one thread each)",
              who, opt.points, Pin, MPX_ROADMAP_MAX_NODES);
  MPX_REQUIRE(opt.passes >= 0, "%s: passes = %d, need >= 0", who, opt.passes);
  MPX_REQUIRE(opt.fanout >= 1 && opt.fanout <= MPX_SHORTCUT_MAX_FANOUT, "%s: fanout = %d, need 1 .. %d", who, opt.fanout,
              MPX_SHORTCUT_MAX_FANOUT);
  MPX_REQUIRE(opt.resolution > 0.0f, "%s: resolution must be > 0", who);
  MPX_REQUIRE(opt.rot_weight > 0.0f && opt.rot_weight < __builtin_inff(), "%s: rot_weight must be > 0 and finite", who);
  MPX_REQUIRE(opt.check_margin >= 0.0f, "%s: negative check_margin", who);
  MPX_REQUIRE(opt.clearance == opt.clearance, "%s: clearance is NaN", who);
  return 0;
}
// (NS supports per problem, C kept candidates)
static inline int task_candidates_options_check(const char *who, int NS, int C, const mpx_task_candidates_options &opt) {
  MPX_REQUIRE(opt.draws >= 1 && opt.draws <= MPX_TASK_MAX_DRAWS, "%s: draws = %d, need 1 .. %d (one thread each)", who, opt.draws,
              MPX_TASK_MAX_DRAWS);
  MPX_REQUIRE(C >= 1 && C <= MPX_TASK_MAX_CANDIDATES, "%s: C = %d kept candidates, need 1 .. %d", who, C, MPX_TASK_MAX_CANDIDATES);
  MPX_REQUIRE(NS >= 1 && NS <= MPX_TASK_MAX_SUPPORTS, "%s: NS = %d supports per problem, need 1 .. %d", who, NS,
              MPX_TASK_MAX_SUPPORTS);
  MPX_REQUIRE(opt.role == 0 || opt.role == 1, "%s: role = %d, need 0 (start) or 1 (goal)", who, opt.role);
  MPX_REQUIRE(opt.self_margin >= 0.0f, "%s: negative (or NaN) self_margin", who);
  MPX_REQUIRE(opt.clearance == opt.clearance, "%s: clearance is NaN", who);
  return 0;
}

// (a negative S, M1 or M2 is the entry's own "negative size")
static inline int franka_counts_check(const char *who, int S, int M1 = 0, int M2 = 0) {
  MPX_REQUIRE(S <= MPX_IK_SEEDS, "%s: S = %d collision spheres, at most %d", who, S, MPX_IK_SEEDS);
  MPX_REQUIRE(M1 <= 64 && M2 <= 64, "%s: at most 64 cuboids and 64 cylinders per problem (%d, %d)", who, M1, M2);
  return 0;
}
static inline int franka_sphere_table_check(const char *who, int S, const float *sph_centers, const float *sph_radii,
                                            const int32_t *sph_link) {
  MPX_REQUIRE(S == 0 || (sph_centers && sph_radii && sph_link), "%s: S > 0 without the sphere table", who);
  return 0;
}
static inline int franka_primitive_arrays_check(const char *who, int S, const float *cub_inv_frames, const float *cub_dims,
                                                int M1, const float *cyl_inv_frames, const float *cyl_radii,
                                                const float *cyl_heights, int M2) {
  MPX_REQUIRE(M1 == 0 || (cub_inv_frames && cub_dims), "%s: M1 > 0 without cuboid arrays", who);
  MPX_REQUIRE(M2 == 0 || (cyl_inv_frames && cyl_radii && cyl_heights), "%s: M2 > 0 without cylinder arrays", who);
  MPX_REQUIRE(M1 + M2 == 0 || S > 0, "%s: primitives without collision spheres to test them with", who);
  return 0;
}
static inline int franka_env_offset_check(const char *who, int64_t env_offset, int B) {
  MPX_REQUIRE(env_offset >= 0 && env_offset + B <= 0xFFFFFFFFll, "%s: env_offset + B exceeds 2^32", who);
  return 0;
}

// `cloud_is_read` = false: the entry reads no point (no cloud, or N == 0) and says a short stride is then tolerated
// (mpx_franka_plan_cloud; the cloud-collision entries and mpx_franka_ik_cloud refuse it whatever N is).
static inline int franka_cloud_operand_check(const char *who, int B, int S, int N, float point_radius, float clearance,
                                             int cloud_point_stride, bool cloud_is_read = true) {
  MPX_REQUIRE(B >= 0 && S >= 0 && N >= 0, "%s: negative size", who);
  MPX_REQUIRE(point_radius >= 0.0f, "%s: point_radius must be >= 0", who);
  MPX_REQUIRE(clearance == clearance, "%s: clearance is NaN", who);
  MPX_REQUIRE(cloud_point_stride >= 3 || !cloud_is_read, "%s: cloud_point_stride < 3", who);
  return 0;
}
// the B x T rows (waypoints, starts, refined configurations) an entry indexes in int32; `product` is its name for them
static inline int franka_rows_check(const char *who, int B, int T, const char *product) {
  MPX_REQUIRE(T >= 0, "%s: negative size", who);
  MPX_REQUIRE((int64_t)B * T < (int64_t)1 << 31, "%s: %s overflows int32", who, product);
  return 0;
}

// `need` is what the entry's own <who>_scratch(dims...) answers
static inline int franka_scratch_size_check(const char *who, int64_t scratch_bytes, int64_t need, std::initializer_list<int> dims) {
  char args[64] = "";  // (at most four ints of up to 11 characters and their separators)
  int at = 0;
  if (scratch_bytes < need)
    for (int d : dims) at += snprintf(args + at, sizeof(args) - (size_t)at, at ? ", %d" : "%d", d);
  MPX_REQUIRE(scratch_bytes >= need, "%s: scratch of %lld bytes, %s_scratch(%s) = %lld", who, (long long)scratch_bytes, who,
              args, (long long)need);
  return 0;
}
static inline int franka_scratch_pointer_check(const char *who, const void *scratch) {
  MPX_REQUIRE(scratch && (reinterpret_cast<uintptr_t>(scratch) & 15) == 0, "%s: scratch is NULL or not 16-byte aligned", who);
  return 0;
}

// pairs = (waypoint, sphere) pairs of a full chunk -> launch(BLOCK, PPT) as std::integral_constants.  Up to 64 pairs (one
// waypoint: a configuration, the rollout step): one wave, one pair per lane; above, the pairs per thread of 256, rounded to even.
template <class Launch>
static inline void franka_cloud_launch_form(int pairs, Launch &&launch) {
  using B256 = std::integral_constant<int, 256>;
  if (pairs <= 64) return launch(std::integral_constant<int, 64>(), std::integral_constant<int, 1>());
  switch ((pairs + 511) / 512) {
    case 1: return launch(B256(), std::integral_constant<int, 2>());
    case 2: return launch(B256(), std::integral_constant<int, 4>());
    case 3: return launch(B256(), std::integral_constant<int, 6>());
    case 4: return launch(B256(), std::integral_constant<int, 8>());
    case 5: return launch(B256(), std::integral_constant<int, 10>());
    case 6: return launch(B256(), std::integral_constant<int, 12>());
    case 7: return launch(B256(), std::integral_constant<int, 14>());
    default: return launch(B256(), std::integral_constant<int, 16>());
  }
}
