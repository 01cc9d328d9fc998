// follow_miss.inc -- the miss of the last guide pose, the end of the follower's verdict.  Included as a statement block by
// follow.hip and follow_cloud.hip (dls_direction.inc's idiom: as an inline function in follow_device.h it moved both
// kernels' instruction streams, profiles/follow_shared_isa.md).
//   in scope: q[7] (the final state), finger, my_poses, W, opt, int bits
//   updates:  bits |= MPX_FOLLOW_BIT_MISS where right_gripper is farther than its share of miss_tol from the last pose
  {
    Rigid eff;
    franka_fk_visit(q, finger, [&](auto ID, const Rigid &g) __attribute__((always_inline)) {
      if constexpr (decltype(ID)::value == 14) eff = g;
    });
    float Rl[9], pl[3];
    follow_load_pose(my_poses + 16 * (W - 1), Rl, pl);
    if (!(follow_distance(pl, eff) <= opt.miss_tol * MPX_FOLLOW_MISS_SHARE)) bits |= MPX_FOLLOW_BIT_MISS;
  }
