// follow_step_head.inc -- steps 1 to 4 of one time step of the follower: forward kinematics, the switch to the next guide
// pose, the stop at the last one, and the attractor.  Included as a statement block INSIDE the time loop of follow.hip and
// follow_cloud.hip (dls_direction.inc's idiom); step 3 leaves the loop with `break`.  The obstacle term (step 5) is the
// including kernel's own and follows this block.
//   in scope: q[7], finger, link, cx, cy, cz (this lane's collision sphere: the link it rides on, -1 for none, and its
//             centre in that link's frame), Rt[9], pt[3] (the current guide pose), w, nw, fin, W, my_poses, opt, lam2
//   defines:  float o[7][3], z[7][3] (origin and z axis of the seven joint frames), sx, sy, sz (this lane's sphere centre
//             in the world), u[7] (the attractor), and what dls_direction.inc defines; advances w, nw, Rt, pt; sets fin
    // 1. FK: the joint origins and axes, right_gripper, and this lane's sphere centre from the frame of its link
    float o[7][3], z[7][3], sx = 0.0f, sy = 0.0f, sz = 0.0f;  // (sx, sy, sz: the sphere centre)
    Rigid eff;
    franka_fk_visit(q, finger, [&](auto ID, const Rigid &g) __attribute__((always_inline)) {
      constexpr int id = decltype(ID)::value;
      if constexpr (id >= 1 && id <= 7) {
        o[id - 1][0] = g.t[0], o[id - 1][1] = g.t[1], o[id - 1][2] = g.t[2];
        z[id - 1][0] = g.r[2], z[id - 1][1] = g.r[5], z[id - 1][2] = g.r[8];
      }
      if constexpr (id == 14) eff = g;
      if constexpr (id >= 1) {
        if (link == id) rigid_apply(g, cx, cy, cz, sx, sy, sz);
      }
    });
    float dist = follow_distance(pt, eff);
    // 2. switch (at most one advance), 3. stop (only where the last pose was the target on entry)
    const bool last_on_entry = w == W - 1;
    if (!last_on_entry && (dist <= opt.switch_radius || nw >= opt.switch_steps)) {
      ++w, nw = 0;
      follow_load_pose(my_poses + 16 * w, Rt, pt);
      dist = follow_distance(pt, eff);
    }
    if (last_on_entry && (dist < opt.final_radius || nw >= opt.final_steps)) {
      fin = 1;
      break;
    }
    // 4. the attractor: mpx_franka_ik's dq
#define DLS_STEP_CLIP opt.step_clip
#include "dls_direction.inc"
#undef DLS_STEP_CLIP
    float u[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) u[j] = dq[j] * scale;
